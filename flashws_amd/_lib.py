"""ctypes binding of libfws_gpu.so (include/fws_gpu.h).

Loads the in-tree build (flashws_amd/lib/libfws_gpu.so) and fails loudly when
it is missing: there is no CPU fallback anywhere on the product path.

torch is imported first on purpose: it loads its bundled libamdhip64.so.7 and
libfws_gpu.so then binds to that same HIP runtime (same SONAME), so torch
tensors' device pointers and torch streams are valid handles for the ABI.
"""
import ctypes as C
import os

import numpy as np

try:  # noqa: SIM105 - see module docstring
    import torch  # noqa: F401
except ImportError:  # pragma: no cover - torch is part of the image
    torch = None

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# FWS_LIB_VARIANT=<tag> loads an in-tree A/B build, lib/libfws_gpu_<tag>.so (make exp), e.g. to run
# the parity tests on an experimental kernel; unset, the product library
_VARIANT = os.environ.get("FWS_LIB_VARIANT", "")
LIB_PATH = os.path.join(PKG_DIR, "lib", f"libfws_gpu_{_VARIANT}.so" if _VARIANT else "libfws_gpu.so")

FWS_OK = 0
FWS_ERR_RSV = -1
FWS_ERR_TOO_LARGE = -2
FWS_ERR_NOT_MASKED = -3
FWS_ERR_MASKED = -4
FWS_ERR_OPCODE = -9
FWS_ERR_CONTROL_FRAME = -10
FWS_ERR_SEQUENCE = -11
FWS_ERR_CAPACITY = -20
FWS_ERR_INVALID = -21
FWS_ERR_NO_DEVICE = -22
FWS_ERR_INTERNAL = -23
FWS_ERR_DECLINED = -24
FWS_ERR_HIP_BASE = -1000

# include/fws_gpu.h structs as numpy dtypes (device arrays are torch uint8 views)
FRAME_DESC = np.dtype([("payload_off", "<u8"), ("payload_len", "<u8"), ("key", "<u4"),
                       ("phase", "<u4")])
FRAME_INFO = np.dtype([("hdr_off", "<u8"), ("payload_len", "<u8"), ("key", "<u4"),
                       ("opcode", "u1"), ("fin", "u1"), ("hdr_len", "u1"), ("flags", "u1")])
DECODE_RESULT = np.dtype([("status", "<i4"), ("n_frames", "<u4"), ("consumed", "<u8"),
                          ("err_off", "<u8"), ("carry_unread", "<u8"), ("carry_hdr_len", "<u4"),
                          ("n_survivors", "<u4")])
MSG_INFO = np.dtype([("off", "<u8"), ("len", "<u8"), ("first_frame", "<u4"), ("last_frame", "<u4"),
                     ("n_data_frames", "<u4"), ("opcode", "u1"), ("utf8_ok", "u1"), ("flags", "u1"), ("pad", "u1")])
MSG_RESULT = np.dtype([("status", "<i4"), ("n_msgs", "<u4"), ("err_frame", "<u4"), ("open_first_frame", "<u4"),
                       ("open_opcode", "<u4"), ("n_data_frames", "<u4"), ("data_bytes", "<u8"),
                       ("ctl_bytes", "<u8"), ("open_off", "<u8"), ("open_len", "<u8"), ("resume_off", "<u8")])
assert MSG_INFO.itemsize == 32 and MSG_RESULT.itemsize == 64
FWS_MSG_CONTINUED = 1   # fws_msg_info.flags (fws_gpu_decode_messages_carry)
MSG_CARRY = np.dtype([("open_opcode", "<u4"), ("open_frames", "<u4"), ("open_bytes", "<u8"), ("utf8_tail", "<u4"),
                      ("utf8_bad", "<u4"), ("prev_open_opcode", "<u4"), ("prev_open_frames", "<u4"),
                      ("prev_open_bytes", "<u8"), ("wire_bytes", "<u8"), ("n_msgs", "<u8"), ("reserved", "<u8")])
assert MSG_CARRY.itemsize == 64
# fws_gpu_decode_messages_multi: a read's limits and its descriptor
FWS_MSG_MULTI_MAX_READ = 128 << 10
FWS_MSG_MULTI_MAX_FRAMES = 256
MSG_READ = np.dtype([("wire_off", "<u8"), ("dst_off", "<u8"), ("ctl_off", "<u8"), ("len", "<u4"), ("conn", "<u4"),
                     ("dst_cap", "<u4"), ("ctl_cap", "<u4"), ("frame_base", "<u4"), ("frame_cap", "<u4"),
                     ("msg_base", "<u4"), ("msg_cap", "<u4"), ("reserved", "<u8")])
assert MSG_READ.itemsize == 64
# fws_gpu_decode_messages_flow: the connection's state, fws_msg_carry (the fields of MSG_CARRY) and the frame in
# progress; FWS_MSG_FLOW_MAX_PENDING bounds what a call leaves unconsumed (a partial header or a cut control frame)
MSG_FLOW = np.dtype([("msg", MSG_CARRY), ("frame_unread", "<u8"), ("frame_len", "<u8"), ("frame_key", "<u4"),
                     ("frame_fin", "u1"), ("pad", "u1", (3,)), ("reserved", "<u8")])
assert MSG_FLOW.itemsize == 96 and MSG_FLOW.fields["frame_unread"][1] == MSG_CARRY.itemsize
FWS_MSG_FLOW_MAX_PENDING = 14 + 125 - 1
RX_EVENT = np.dtype([("kind", "<u4"), ("opcode", "<u4"), ("is_ctl", "u1"), ("frame_end", "u1"),
                     ("msg_end", "u1"), ("fin", "u1"), ("code", "<u4"), ("size", "<u8"),
                     ("data_off", "<u8"), ("ctl_off", "<u8"), ("capacity", "<u8")])
TX_DESC = np.dtype([("src_off", "<u8"), ("len", "<u8"), ("key", "<u4"), ("opcode", "u1"), ("fin", "u1"),
                    ("masked", "u1"), ("pad", "u1")])
assert FRAME_DESC.itemsize == 24 and FRAME_INFO.itemsize == 24 and TX_DESC.itemsize == 24
# fws_gpu_encode_messages_multi: a send's limits, the fragment key, the connection's state, the send and its result
FWS_TX_MULTI_MAX_SEND = 128 << 10
FWS_TX_MULTI_MAX_FRAMES = 256


def FWS_TX_FRAG_KEY(key, j):
    return (key + j * 0x9E3779B9) & 0xFFFFFFFF


TX_CONN = np.dtype([("last_msg_not_fin", "<u4"), ("reserved0", "<u4"), ("frames", "<u8"), ("wire_bytes", "<u8"),
                    ("reserved", "<u8")])
TX_SEND = np.dtype([("src_off", "<u8"), ("out_off", "<u8"), ("len", "<u4"), ("out_cap", "<u4"), ("conn", "<u4"),
                    ("max_frame", "<u4"), ("key", "<u4"), ("frame_type", "u1"), ("last", "u1"), ("masked", "u1"),
                    ("pad", "u1"), ("frame_base", "<u4"), ("frame_cap", "<u4"), ("reserved", "<u8", (2,))])
TX_RESULT = np.dtype([("status", "<i4"), ("n_frames", "<u4"), ("out_len", "<u8"), ("last_msg_not_fin", "<u4"),
                      ("pad", "<u4"), ("reserved", "<u8")])
assert TX_CONN.itemsize == 32 and TX_SEND.itemsize == 64 and TX_RESULT.itemsize == 32
# fws_gpu_reply_messages_multi: what is answered, the connection's reply state and a read's output region
FWS_REPLY_CONTROL = 1   # PING -> PONG, CLOSE -> CLOSE
FWS_REPLY_ECHO = 2      # every data part goes back as one frame
REPLY_STATE = np.dtype([("close_sent", "<u4"), ("close_code", "<u4"), ("fail_code", "<u4"), ("reserved", "<u4")])
REPLY_REGION = np.dtype([("out_off", "<u8"), ("out_cap", "<u4"), ("frame_base", "<u4"), ("frame_cap", "<u4"),
                         ("reserved0", "<u4"), ("reserved", "<u8")])
assert REPLY_STATE.itemsize == 16 and REPLY_REGION.itemsize == 32
# fws_gpu_reply_messages_strict: the status codes of the CLOSE that fails a connection (RFC 6455 §7.4.1)
FWS_CLOSE_PROTOCOL_ERROR = 1002   # a malformed CLOSE, a bad status code, a decode that ended in a protocol error
FWS_CLOSE_INVALID_DATA = 1007     # a TEXT message or a CLOSE reason that is not UTF-8
FWS_CLOSE_TOO_BIG = 1009          # a message over max_message_bytes, a frame over 2^32 bytes
# the decode statuses answered with 1002; FWS_ERR_TOO_LARGE is answered with 1009
FWS_PROTOCOL_ERRORS = (FWS_ERR_RSV, FWS_ERR_NOT_MASKED, FWS_ERR_MASKED, FWS_ERR_OPCODE, FWS_ERR_CONTROL_FRAME,
                       FWS_ERR_SEQUENCE)


# fws_gpu_join_messages: where a message lies, the connection's join state, an entry's record and a read's result
FWS_JOIN_IN_DST = 0     # whole in this read: dev_dst, not copied
FWS_JOIN_IN_STORE = 1   # joined in the connection's slot of dev_store
FWS_JOIN_IN_CTL = 2     # a control frame: dev_ctl
FWS_JOIN_NOWHERE = 3    # dropped: longer than half a slot
FWS_JOIN_DROPPED = 1    # fws_join_info.flags
JOIN_STATE = np.dtype([("open_opcode", "<u4"), ("half", "<u4"), ("dropped", "<u4"), ("reserved0", "<u4"),
                       ("open_bytes", "<u8"), ("fill", "<u8")])
JOIN_INFO = np.dtype([("off", "<u8"), ("len", "<u8"), ("opcode", "u1"), ("utf8_ok", "u1"), ("where", "u1"),
                      ("flags", "u1"), ("reserved0", "<u4"), ("reserved", "<u8")])
JOIN_RESULT = np.dtype([("status", "<i4"), ("n_joined", "<u4"), ("copied", "<u8"), ("open_opcode", "<u4"),
                        ("dropped", "<u4"), ("reserved", "<u8")])
assert JOIN_STATE.itemsize == 32 and JOIN_INFO.itemsize == 32 and JOIN_RESULT.itemsize == 32
# fws_gpu_publish_messages: the records one subscriber's list may name and a subscriber's descriptor
FWS_PUB_MAX_ITEMS = 256
PUB_SUB = np.dtype([("out_off", "<u8"), ("out_cap", "<u4"), ("conn", "<u4"), ("list_off", "<u4"), ("list_len", "<u4"),
                    ("frame_base", "<u4"), ("frame_cap", "<u4")])
assert PUB_SUB.itemsize == 32


def close_code_valid(code):
    """Whether a status code may appear in a CLOSE frame: the registry as of RFC 6455 plus 1012-1014."""
    return 1000 <= code <= 1003 or 1007 <= code <= 1014 or 3000 <= code <= 4999


assert DECODE_RESULT.itemsize == 40 and RX_EVENT.itemsize == 48
RX_READ = np.dtype([("conn", "<u4"), ("flags", "<u4"), ("buf", "<u8"), ("size", "<u8"), ("capacity", "<u8")])
RX_READ_RESULT = np.dtype([("ret", "<i4"), ("pad", "<u4"), ("events", "<u8"), ("n_events", "<u8"),
                           ("ctl", "<u8"), ("ctl_used", "<u8")])
assert RX_READ.itemsize == 32 and RX_READ_RESULT.itemsize == 40
DECODE_JOB = np.dtype([("wire", "<u8"), ("len", "<u8"), ("frames", "<u8"), ("cap", "<u4"), ("reserved", "<u4"),
                       ("result", "<u8"), ("utf8_ok", "<u8")])
assert DECODE_JOB.itemsize == 48


class RxState(C.Structure):
    """fws_rx_state (field names of the reference's members, w_socket.h:223-245)."""
    _fields_ = [("recv_status", C.c_int32), ("last_rx_mask_key", C.c_uint32),
                ("unread_pl_len", C.c_uint64), ("last_rx_opcode", C.c_uint8),
                ("last_rx_control_opcode", C.c_uint8), ("last_rx_fin_flag", C.c_uint8),
                ("is_rx_control_frame", C.c_uint8), ("last_rx_hdr_part_len", C.c_uint32)]


class GenParams(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("kind", C.c_uint32), ("opcode", C.c_uint32),
                ("n_frames", C.c_uint64), ("payload_min", C.c_uint64), ("payload_max", C.c_uint64),
                ("target_bytes", C.c_uint64), ("invalid_permille", C.c_uint32),
                ("pad_", C.c_uint32)]


# (name, restype, argtypes) for every symbol include/fws_gpu.h declares
_P, _U32, _U64, _I = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
_PU64 = C.POINTER(C.c_uint64)
SIGNATURES = [
    ("fws_gpu_abi_version", _I, []),
    ("fws_gpu_device_count", _I, [C.POINTER(C.c_int)]),
    ("fws_gpu_ctx_create", _I, [_I, C.POINTER(C.c_void_p)]),
    ("fws_gpu_ctx_destroy", None, [_P]),
    ("fws_gpu_ctx_reserve", _I, [_P, _U64, _U64]),
    ("fws_gpu_ctx_set_rx_persistent", _I, [_P, _U32]),
    ("fws_gpu_mask", _I, [_P, _U64, _U32, _P]),
    ("fws_gpu_unmask_batch", _I, [_P, _P, _P, _U32, _P]),
    ("fws_gpu_unmask_sorted", _I, [_P, _P, _P, _U32, _P]),
    ("fws_gpu_unmask_sorted_utf8", _I, [_P, _P, _P, _U32, _P, _P]),
    ("fws_gpu_unmask_plan", _I, [_P, _P, _P, _U32, _P]),
    ("fws_gpu_unmask_run", _I, [_P, _P, _P, _U32, _P]),
    ("fws_gpu_unmask_gather", _I, [_P, _P, _P, _P, _U32, _P]),
    ("fws_gpu_decode_stream", _I, [_P, _P, _U64, _P, _U32, _P, _P, _P]),
    ("fws_gpu_decode_messages", _I, [_P, _P, _U64, _P, _U32, _P, _U32, _P, _U64, _P, _U64, _P, _P, _P]),
    ("fws_gpu_decode_messages_carry", _I, [_P, _P, _U64, _P, _U32, _P, _U32, _P, _U64, _P, _U64, _P, _P, _P, _P]),
    ("fws_gpu_decode_messages_multi", _I, [_P, _P, _P, _U32, _U32, _P, _P, _P, _P, _P, _P, _P, _U32, _P]),
    ("fws_gpu_decode_messages_flow", _I, [_P, _P, _P, _U32, _U32, _P, _P, _P, _P, _P, _P, _P, _U32, _P]),
    ("fws_gpu_decode_messages_flow_client", _I, [_P, _P, _P, _U32, _U32, _P, _P, _P, _P, _P, _P, _P, _U32, _P]),
    ("fws_gpu_validate_utf8", _I, [_P, _P, _P, _U32, _P, _P]),
    ("fws_rx_session_create", _I, [_P, _I, C.POINTER(C.c_void_p)]),
    ("fws_rx_session_destroy", None, [_P]),
    ("fws_rx_session_feed", _I, [_P, _P, _U64, _U64, _P, _U64, _PU64, _P, _U64, _PU64]),
    ("fws_rx_session_state", _I, [_P, _P]),
    ("fws_rx_session_feed_view", _I, [_P, _P, _U64, _U64, C.POINTER(C.c_void_p), _PU64, C.POINTER(C.c_void_p),
                                      _PU64]),
    ("fws_rx_session_error", _I, [_P, C.POINTER(C.c_uint32)]),
    ("fws_gpu_check_sorted", _I, [_P, _P, _U32, _P, _P]),
    ("fws_rx_mux_create", _I, [_P, _U32, C.POINTER(C.c_void_p)]),
    ("fws_rx_mux_destroy", None, [_P]),
    ("fws_rx_mux_reset", _I, [_P, _U32]),
    ("fws_rx_mux_state", _I, [_P, _U32, _P]),
    ("fws_rx_mux_error", _I, [_P, _U32, C.POINTER(C.c_uint32)]),
    ("fws_rx_mux_feed", _I, [_P, _P, _U32, _P]),
    ("fws_rx_mux_submit", _I, [_P, _P, _U32]),
    ("fws_rx_mux_complete", _I, [_P, _P]),
    ("fws_rx_mux_ready", _I, [_P]),
    ("fws_gen_batch", _I, [C.POINTER(GenParams), _P, _U64, _PU64, _P, _U64, _PU64, _P]),
    ("fws_tx_next", None, [_U32, _I, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8)]),
    ("fws_gpu_encode_frames", _I, [_P, _P, _U64, _P, _P, _U32, _P, _P]),
    ("fws_gpu_encode_messages_multi", _I, [_P, _P, _P, _P, _U32, _U32, _P, _P, _P, _U32, _P]),
    ("fws_gpu_reply_messages_multi", _I, [_P, _P, _U32, _U32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _U32, _U32,
                                          _P]),
    ("fws_gpu_reply_messages_strict", _I, [_P, _P, _U32, _U32, _P, _P, _P, _P, _P, _U32, _U64, _P, _P, _P, _P, _P, _P,
                                           _U32, _U32, _P]),
    ("fws_gpu_reply_messages_multi_client", _I, [_P, _P, _U32, _U32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _U32, _U32,
                                                 _P, _P]),
    ("fws_gpu_reply_messages_strict_client", _I, [_P, _P, _U32, _U32, _P, _P, _P, _P, _P, _U32, _U64, _P, _P, _P, _P,
                                                  _P, _P, _U32, _U32, _P, _P]),
    ("fws_gpu_join_messages", _I, [_P, _P, _U32, _U32, _P, _P, _P, _P, _U64, _P, _P, _P, _U32, _P]),
    ("fws_gpu_publish_messages", _I, [_P, _P, _U32, _P, _P, _P, _P, _U32, _P, _U32, _U32, _P, _P, _P, _P, _P, _U32,
                                      _P]),
    ("fws_tx_session_create", _I, [_P, _I, C.POINTER(C.c_void_p)]),
    ("fws_tx_session_destroy", None, [_P]),
    ("fws_tx_session_send", _I, [_P, _P, _P, _P, _P, _P, _U32, _P, _U64, _PU64]),
    ("fws_tx_session_state", _I, [_P, C.POINTER(C.c_uint8)]),
    ("fws_gpu_host_register", _I, [_P, _U64]),
    ("fws_gpu_host_unregister", _I, [_P]),
    ("fws_rx_pipe_create", _I, [_I, _U64, _U32, _U32, _I, C.POINTER(C.c_void_p)]),
    ("fws_rx_pipe_destroy", None, [_P]),
    ("fws_rx_pipe_submit", _I, [_P, _P, _U64, _PU64]),
    ("fws_rx_pipe_wait", _I, [_P, _U64, C.POINTER(C.c_void_p), _PU64, _P, C.POINTER(C.c_void_p)]),
    ("fws_decode_engine_create", _I, [_I, _U64, _U64, C.POINTER(C.c_void_p)]),
    ("fws_decode_engine_destroy", None, [_P]),
    ("fws_decode_engine_run", _I, [_P, _P, _U32, _P]),
]

_lib = None


class FwsError(RuntimeError):
    def __init__(self, fn, code):
        super().__init__(f"{fn} failed with status {code}")
        self.code = code


def lib():
    """The loaded library. Raises if the in-tree build is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
                f"g.build()'` (make -C flashws_amd/csrc). There is no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        for name, res, args in SIGNATURES:
            fn = getattr(L, name, None)
            if fn is None:
                continue  # reported by exported_symbols(); callers fail on use
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def exported_symbols():
    """Names from SIGNATURES that the library actually exports."""
    L = lib()
    return [n for n, _, _ in SIGNATURES if hasattr(L, n)]


def check(fn, code):
    if code != 0:
        raise FwsError(fn, code)
    return code
