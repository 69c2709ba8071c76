// reply_strict_client_kernels.hip -- fws_gpu_reply_messages_strict_client:
// k_reply_strict's masked instantiations (reply_strict_kernels.hip, kMasked)
// and their launch, in a translation unit of their own as
// reply_client_kernels.hip.
#define FWS_REPLY_CLIENT_TU 1
#include "reply_strict_kernels.hip"
