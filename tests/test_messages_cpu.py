"""CPU: the ABI surface of fws_gpu_decode_messages -- the symbol, the struct
layouts of fws_msg_info / fws_msg_result against the header comments and the
numpy mirrors, the new status code, and the argument checks that come before
any device call. No device calls."""
import ctypes as C
import os
import re

from flashws_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fws_gpu.h")


def test_symbol_is_exported_and_bound():
    L = _lib.lib()
    assert hasattr(L, "fws_gpu_decode_messages")
    assert "fws_gpu_decode_messages" in _lib.exported_symbols()
    sig = {n: a for n, _, a in _lib.SIGNATURES}["fws_gpu_decode_messages"]
    assert len(sig) == 14


def test_struct_sizes_match_header_comments_and_dtypes():
    src = open(HEADER).read()
    sizes = dict(re.findall(r"\}\s*(fws_[a-z_]+);\s*/\*\s*(\d+) bytes", src))
    assert int(sizes["fws_msg_info"]) == _lib.MSG_INFO.itemsize == 32
    assert int(sizes["fws_msg_result"]) == _lib.MSG_RESULT.itemsize == 64


def test_struct_fields_follow_the_header_order():
    src = open(HEADER).read()
    for name, dt in (("fws_msg_info", _lib.MSG_INFO), ("fws_msg_result", _lib.MSG_RESULT)):
        body = re.search(r"typedef struct %s \{(.*?)\}" % name, src, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = re.findall(r"\b(?:u?int\d+_t)\s+([a-z0-9_]+)\s*;", body)
        widths = [int(w) // 8 for w in re.findall(r"\bu?int(\d+)_t\s+[a-z0-9_]+\s*;", body)]
        assert list(dt.names) == fields, name
        assert [dt.fields[f][0].itemsize for f in fields] == widths, name
        # natural alignment, no hidden padding
        off = 0
        for f, w in zip(fields, widths):
            assert dt.fields[f][1] == off and off % w == 0, (name, f)
            off += w


def test_sequence_status_code():
    assert _lib.FWS_ERR_SEQUENCE == -11
    src = open(HEADER).read()
    assert re.search(r"FWS_ERR_SEQUENCE\s*=\s*-11\b", src)
    assert re.search(r"FWS_ERR_CONTROL_FRAME\s*=\s*-10\b", src)


def test_invalid_arguments_fail_before_any_device_call():
    L = _lib.lib()
    f = L.fws_gpu_decode_messages
    # stand-ins for pointers the checks must never follow
    page = (C.c_uint8 * 8192)()
    base = (C.addressof(page) + 4095) & ~4095
    ctx, wire, dst = base, base + 1024, base + 2048
    frames, msgs, ctl, res, mres = (base + 4096 + 64 * i for i in range(5))
    ok = [ctx, wire, 0, frames, 4, msgs, 4, dst, 64, ctl, 64, res, mres, None]

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[{"ctx": 0, "wire": 1, "n": 2, "dst": 7, "res": 11, "mres": 12}[k]] = v
        return f(*a)

    assert call(ctx=None) == _lib.FWS_ERR_INVALID
    assert call(mres=None) == _lib.FWS_ERR_INVALID
    assert call(res=None) == _lib.FWS_ERR_INVALID
    assert call(dst=dst + 8) == _lib.FWS_ERR_INVALID
    assert call(wire=wire + 4, n=16) == _lib.FWS_ERR_INVALID
    assert call(wire=None, n=16) == _lib.FWS_ERR_INVALID
