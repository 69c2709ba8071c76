// reply_client_kernels.hip -- fws_gpu_reply_messages_multi_client: k_reply's
// masked instantiations (reply_kernels.hip, kMasked) and their launch, in a
// translation unit of their own so that the unmasked kernels' code stays what
// it was (see there).
#define FWS_REPLY_CLIENT_TU 1
#include "reply_kernels.hip"
