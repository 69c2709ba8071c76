"""CPU: the ABI surface of fws_gpu_decode_messages_carry -- the symbol, the
layout of fws_msg_carry against the header and the numpy mirror, the
FWS_MSG_CONTINUED flag, and the argument checks that come before any device
call. And the GPU test's inputs and oracle, on the CPU: the oracle's UTF-8
rules against bytes.decode, its cut invariant against itself, and the condition
test_random_streams puts on its 40 seeds. No device calls."""
import ctypes as C
import os
import random
import re

import test_gpu_msg_carry as carry_cases
from flashws_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fws_gpu.h")


def test_symbol_is_exported_and_bound():
    L = _lib.lib()
    assert hasattr(L, "fws_gpu_decode_messages_carry")
    assert "fws_gpu_decode_messages_carry" in _lib.exported_symbols()
    sig = {n: a for n, _, a in _lib.SIGNATURES}
    assert len(sig["fws_gpu_decode_messages_carry"]) == 15
    # every argument of fws_gpu_decode_messages, then the carry, then the stream
    old = sig["fws_gpu_decode_messages"]
    assert sig["fws_gpu_decode_messages_carry"] == old[:-1] + [C.c_void_p, old[-1]]


def test_carry_is_64_bytes_in_the_header_order_without_padding():
    src = open(HEADER).read()
    sizes = dict(re.findall(r"\}\s*(fws_[a-z_]+);\s*/\*\s*(\d+) bytes", src))
    assert int(sizes["fws_msg_carry"]) == _lib.MSG_CARRY.itemsize == 64
    body = re.search(r"typedef struct fws_msg_carry \{(.*?)\}", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(?:u?int\d+_t)\s+([a-z0-9_]+)\s*;", body)
    widths = [int(w) // 8 for w in re.findall(r"\bu?int(\d+)_t\s+[a-z0-9_]+\s*;", body)]
    dt = _lib.MSG_CARRY
    assert fields == ["open_opcode", "open_frames", "open_bytes", "utf8_tail", "utf8_bad", "prev_open_opcode",
                      "prev_open_frames", "prev_open_bytes", "wire_bytes", "n_msgs", "reserved"]
    assert list(dt.names) == fields
    assert [dt.fields[f][0].itemsize for f in fields] == widths
    off = 0
    for f, w in zip(fields, widths):
        assert dt.fields[f][1] == off and off % w == 0, f
        off += w
    assert off == 64


def test_existing_structs_and_the_abi_version_did_not_move():
    src = open(HEADER).read()
    sizes = dict(re.findall(r"\}\s*(fws_[a-z_]+);\s*/\*\s*(\d+) bytes", src))
    assert (int(sizes["fws_msg_info"]), int(sizes["fws_msg_result"])) == (32, 64)
    assert _lib.MSG_INFO.itemsize == 32 and _lib.MSG_RESULT.itemsize == 64
    assert re.search(r"#define\s+FWS_GPU_ABI_VERSION\s+1\b", src)
    assert _lib.lib().fws_gpu_abi_version() == 1


def test_continued_flag():
    assert _lib.FWS_MSG_CONTINUED == 1
    assert re.search(r"#define\s+FWS_MSG_CONTINUED\s+1u\b", open(HEADER).read())


def test_invalid_arguments_fail_before_any_device_call():
    L = _lib.lib()
    f = L.fws_gpu_decode_messages_carry
    # stand-ins for pointers the checks must never follow
    page = (C.c_uint8 * 8192)()
    base = (C.addressof(page) + 4095) & ~4095
    ctx, wire, dst = base, base + 1024, base + 2048
    frames, msgs, ctl, res, mres, carry = (base + 4096 + 64 * i for i in range(6))
    ok = [ctx, wire, 0, frames, 4, msgs, 4, dst, 64, ctl, 64, res, mres, carry, None]

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[{"ctx": 0, "wire": 1, "n": 2, "dst": 7, "res": 11, "mres": 12, "carry": 13}[k]] = v
        return f(*a)

    assert call(carry=None) == _lib.FWS_ERR_INVALID
    assert call(ctx=None) == _lib.FWS_ERR_INVALID
    assert call(mres=None) == _lib.FWS_ERR_INVALID
    assert call(res=None) == _lib.FWS_ERR_INVALID
    assert call(dst=dst + 8) == _lib.FWS_ERR_INVALID
    assert call(wire=wire + 4, n=16) == _lib.FWS_ERR_INVALID
    assert call(wire=None, n=16) == _lib.FWS_ERR_INVALID


def test_the_oracles_utf8_rules_are_utf8():
    """Rules (A) and (B) flag nothing in b + 3 zero bytes iff b decodes strictly."""
    rng = random.Random(1)
    pool = [0x00, 0x41, 0x7F, 0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xBF, 0xC0, 0xC1, 0xC2, 0xDF, 0xE0, 0xE1, 0xEC, 0xED,
            0xEE, 0xEF, 0xF0, 0xF1, 0xF3, 0xF4, 0xF5, 0xFF]
    for _ in range(20000):
        b = bytes(rng.choice(pool) for _ in range(rng.randint(0, 6)))
        clean = not any(carry_cases.utf8_flagged(b, j) for j in range(len(b) + 3))
        assert clean == bool(carry_cases.strict_ok(b)), b


def test_all_40_random_seeds_make_two_calls_and_deliver_a_continued_entry():
    for seed in range(40):
        calls, continued, units = carry_cases.reference_walk(seed)
        assert calls >= 2 and continued >= 1, seed
        wire, cuts = carry_cases.random_cuts(seed)
        assert units == carry_cases.whole(wire)[0], seed


def test_the_oracle_delivers_the_same_units_for_every_cut():
    stream = carry_cases.twelve_frames()
    units, status, _ = carry_cases.whole(stream)
    assert status == 0 and len(units) == 8
    for cut in range(len(stream) + 1):
        ref, pos, got = carry_cases.RefConn(), 0, []
        for b in (cut, len(stream)):
            out = ref.call(stream[pos:b])
            pos += out["res"]["resume_off"]
            got += out["units"]
        assert got == units and pos == len(stream), cut
