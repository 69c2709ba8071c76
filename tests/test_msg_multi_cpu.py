"""CPU: the ABI surface of fws_gpu_decode_messages_multi -- the symbol, the
layout of fws_msg_read against the header and the numpy mirror, the new status
code and the two limits, and the argument checks that come before any device
call. No device calls."""
import ctypes as C
import os
import re

from flashws_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fws_gpu.h")
NAME = "fws_gpu_decode_messages_multi"


def test_symbol_is_exported_and_bound():
    L = _lib.lib()
    assert hasattr(L, NAME)
    assert NAME in _lib.exported_symbols()
    sig = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    res, args = sig[NAME]
    assert res is C.c_int and len(args) == 14
    # ctx, wire, reads, n, max_len, 7 arrays, n_conns, stream
    assert args[3] is C.c_uint32 and args[4] is C.c_uint32 and args[12] is C.c_uint32
    assert all(a is C.c_void_p for i, a in enumerate(args) if i not in (3, 4, 12))


def test_read_descriptor_is_64_bytes_in_the_header_order_without_padding():
    src = open(HEADER).read()
    sizes = dict(re.findall(r"\}\s*(fws_[a-z_]+);\s*/\*\s*(\d+) bytes", src))
    assert int(sizes["fws_msg_read"]) == _lib.MSG_READ.itemsize == 64
    body = re.search(r"typedef struct fws_msg_read \{(.*?)\}", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields, widths = [], []
    for w, names in re.findall(r"\bu?int(\d+)_t\s+([a-z0-9_, ]+);", body):
        for nm in names.split(","):
            fields.append(nm.strip())
            widths.append(int(w) // 8)
    dt = _lib.MSG_READ
    assert fields == ["wire_off", "dst_off", "ctl_off", "len", "conn", "dst_cap", "ctl_cap", "frame_base", "frame_cap",
                      "msg_base", "msg_cap", "reserved"]
    assert list(dt.names) == fields
    assert [dt.fields[f][0].itemsize for f in fields] == widths
    off = 0
    for f, w in zip(fields, widths):
        assert dt.fields[f][1] == off and off % w == 0, f
        off += w
    assert off == 64


def test_declined_code_and_the_limits():
    src = open(HEADER).read()
    assert _lib.FWS_ERR_DECLINED == -24
    assert re.search(r"\bFWS_ERR_DECLINED\s*=\s*-24\b", src)
    assert _lib.FWS_MSG_MULTI_MAX_READ == 128 << 10 and _lib.FWS_MSG_MULTI_MAX_FRAMES == 256
    assert re.search(r"#define\s+FWS_MSG_MULTI_MAX_READ\s+\(128u\s*<<\s*10\)", src)
    assert re.search(r"#define\s+FWS_MSG_MULTI_MAX_FRAMES\s+256u\b", src)
    codes = [v for k, v in vars(_lib).items() if k.startswith("FWS_ERR_")]
    assert len(codes) == len(set(codes))


def test_existing_structs_and_the_abi_version_did_not_move():
    src = open(HEADER).read()
    sizes = {k: int(v) for k, v in re.findall(r"\}\s*(fws_[a-z_]+);\s*/\*\s*(\d+) bytes", src)}
    assert (sizes["fws_frame_desc"], sizes["fws_frame_info"], sizes["fws_decode_result"]) == (24, 24, 40)
    assert (sizes["fws_msg_info"], sizes["fws_msg_result"], sizes["fws_msg_carry"]) == (32, 64, 64)
    assert (_lib.FRAME_INFO.itemsize, _lib.DECODE_RESULT.itemsize) == (24, 40)
    assert (_lib.MSG_INFO.itemsize, _lib.MSG_RESULT.itemsize, _lib.MSG_CARRY.itemsize) == (32, 64, 64)
    assert re.search(r"#define\s+FWS_GPU_ABI_VERSION\s+1\b", src)
    assert _lib.lib().fws_gpu_abi_version() == 1
    for name, code in (("FWS_ERR_CAPACITY", -20), ("FWS_ERR_INVALID", -21), ("FWS_ERR_INTERNAL", -23)):
        assert getattr(_lib, name) == code and re.search(rf"\b{name}\s*=\s*{code}\b", src)


def stand_ins():
    """Pointers the checks must never follow: addresses inside one host page pair."""
    page = (C.c_uint8 * 8192)()
    base = (C.addressof(page) + 4095) & ~4095
    ctx, wire, dst = base, base + 1024, base + 2048
    reads, frames, msgs, ctl, res, mres, carries = (base + 4096 + 64 * i for i in range(7))
    ok = [ctx, wire, reads, 4, 4096, frames, msgs, dst, ctl, res, mres, carries, 4, None]
    return page, ok


INDEX = {"ctx": 0, "wire": 1, "reads": 2, "n": 3, "max_len": 4, "frames": 5, "msgs": 6, "dst": 7, "ctl": 8, "res": 9,
         "mres": 10, "carries": 11, "n_conns": 12}


def test_invalid_arguments_fail_before_any_device_call():
    f = getattr(_lib.lib(), NAME)
    page, ok = stand_ins()

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[INDEX[k]] = v
        return f(*a)

    for k in ("ctx", "wire", "reads", "frames", "msgs", "dst", "ctl", "res", "mres", "carries"):
        assert call(**{k: None}) == _lib.FWS_ERR_INVALID, k
    assert call(wire=ok[1] + 4) == _lib.FWS_ERR_INVALID
    assert call(dst=ok[7] + 8) == _lib.FWS_ERR_INVALID
    assert call(max_len=0) == _lib.FWS_ERR_INVALID
    assert call(max_len=_lib.FWS_MSG_MULTI_MAX_READ + 1) == _lib.FWS_ERR_INVALID
    assert call(max_len=0xFFFFFFFF) == _lib.FWS_ERR_INVALID
    del page


def test_no_reads_is_no_launch():
    f = getattr(_lib.lib(), NAME)
    page, ok = stand_ins()
    a = list(ok)
    a[INDEX["n"]] = 0
    assert f(*a) == 0
    # nothing is looked at with n == 0, not even the arguments that would be refused
    assert f(*([None] * 3 + [0, 0] + [None] * 7 + [0, None])) == 0
    del page
