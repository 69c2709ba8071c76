"""CPU: the ABI surface of fws_gpu_reply_messages_strict -- the symbol, its 20
arguments, fws_reply_state against the header and the numpy mirror, the
argument checks that come before any device call -- and StrictRef (fail_ref.py),
the GPU tests' predictor, against a hand-written case list: one line per row of
the header's failure table and per non-failure beside it, the expected reply
spelled as hex. No device calls."""
import ctypes as C
import os
import random
import re
import struct

import test_gpu_msg_carry as cc
import test_reply_cpu as plain
from fail_ref import StrictRef, close_failure, code_valid
from flashws_amd import _lib, gpu
from msgflow_ref import FlowRef
from reply_ref import CONTROL, ECHO, ReplyRef
from wsframes import frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fws_gpu.h")
NAME = "fws_gpu_reply_messages_strict"
TEXT, BIN, CONT, CLOSE, PING, PONG = 1, 2, 0, 8, 9, 10
BOTH = CONTROL | ECHO
K = 0x5A3C9F17                                           # a key with four distinct bytes


def close(code=None, reason=b""):
    return frame(CLOSE, (b"" if code is None else struct.pack(">H", code)) + reason, key=K)


# (name, the connection's reads, flags, max_message_bytes, the reply as hex, fail_code)
CASES = [
    # ---- CLOSE entries
    ("close 1000", [bytes.fromhex("8882 179F3C5A 1477")], BOTH, 0, "88 02 03 E8", 0),   # 88 82 key 03 E8
    ("close empty", [close()], BOTH, 0, "88 00", 0),
    ("close of one byte", [frame(CLOSE, b"\x03", key=K)], BOTH, 0, "88 02 03 EA", 1002),
    ("close 999", [close(999)], BOTH, 0, "88 02 03 EA", 1002),
    ("close 0", [close(0)], BOTH, 0, "88 02 03 EA", 1002),
    ("close 1003", [close(1003)], BOTH, 0, "88 02 03 EB", 0),
    ("close 1004", [close(1004)], BOTH, 0, "88 02 03 EA", 1002),
    ("close 1005", [close(1005)], BOTH, 0, "88 02 03 EA", 1002),
    ("close 1006", [close(1006)], BOTH, 0, "88 02 03 EA", 1002),
    ("close 1007", [close(1007)], BOTH, 0, "88 02 03 EF", 0),
    ("close 1014", [close(1014)], BOTH, 0, "88 02 03 F6", 0),
    ("close 1015", [close(1015)], BOTH, 0, "88 02 03 EA", 1002),
    ("close 1016", [close(1016)], BOTH, 0, "88 02 03 EA", 1002),
    ("close 2999", [close(2999)], BOTH, 0, "88 02 03 EA", 1002),
    ("close 3000", [close(3000)], BOTH, 0, "88 02 0B B8", 0),
    ("close 4999", [close(4999)], BOTH, 0, "88 02 13 87", 0),
    ("close 5000", [close(5000)], BOTH, 0, "88 02 03 EA", 1002),
    ("close 65535", [close(65535)], BOTH, 0, "88 02 03 EA", 1002),
    ("close with a reason", [close(1000, b"ok")], BOTH, 0, "88 04 03 E8 6F 6B", 0),
    ("close with a two-byte character", [close(1001, b"\xc3\xa9")], BOTH, 0, "88 04 03 E9 C3 A9", 0),
    ("reason C3", [close(1000, b"\xc3")], BOTH, 0, "88 02 03 EF", 1007),
    ("reason cut in its last sequence", [close(1000, b"bye \xe2\x82")], BOTH, 0, "88 02 03 EF", 1007),
    ("reason with a surrogate", [close(1000, b"\xed\xa0\x80")], BOTH, 0, "88 02 03 EF", 1007),
    ("a bad code before a bad reason", [close(1005, b"\xc3")], BOTH, 0, "88 02 03 EA", 1002),
    ("a malformed close without FWS_REPLY_CONTROL", [frame(CLOSE, b"\x03", key=K)], ECHO, 0, "88 02 03 EA", 1002),
    ("a good close without FWS_REPLY_CONTROL", [close(1000)], ECHO, 0, "", 0),
    # ---- TEXT / BIN entries
    ("text C3 28", [frame(TEXT, b"\xc3\x28", key=K)], BOTH, 0, "88 02 03 EF", 1007),
    ("text C3 A9", [frame(TEXT, b"\xc3\xa9", key=K)], BOTH, 0, "81 02 C3 A9", 0),
    ("binary C3 28", [frame(BIN, b"\xc3\x28", key=K)], BOTH, 0, "82 02 C3 28", 0),
    ("text C3 28 with no flag set", [frame(TEXT, b"\xc3\x28", key=K)], 0, 0, "88 02 03 EF", 1007),
    ("text C3 28 in two fragments of one read", [frame(TEXT, b"\xc3", fin=0, key=K) + frame(CONT, b"\x28", key=K)],
     BOTH, 0, "88 02 03 EF", 1007),
    ("a message at the limit", [frame(BIN, b"1234", key=K)], BOTH, 4, "82 04 31 32 33 34", 0),
    ("a message over the limit", [frame(BIN, b"12345", key=K)], BOTH, 4, "88 02 03 F1", 1009),
    ("over the limit and not UTF-8", [frame(TEXT, b"123\xc3\x28", key=K)], BOTH, 4, "88 02 03 F1", 1009),
    ("a control payload over the limit", [frame(PING, b"12345", key=K)], BOTH, 4, "8A 05 31 32 33 34 35", 0),
    ("a continued message at the limit", [frame(BIN, b"12", fin=0, key=K), frame(CONT, b"34", key=K)], BOTH, 4,
     "02 02 31 32 80 02 33 34", 0),
    ("a continued message over the limit", [frame(BIN, b"12", fin=0, key=K), frame(CONT, b"345", key=K)], BOTH, 4,
     "02 02 31 32 88 02 03 F1", 1009),
    # ---- the open part
    ("an open part over the limit", [frame(BIN, b"12345", fin=0, key=K)], BOTH, 4, "88 02 03 F1", 1009),
    ("a header that announces more than the limit", [frame(BIN, b"12345", key=K)[:6]], BOTH, 4, "88 02 03 F1", 1009),
    ("a header that announces the limit", [frame(BIN, b"1234", key=K)[:7]], BOTH, 4, "02 01 31", 0),
    ("an open text part already malformed", [frame(TEXT, b"\xc3\x28", fin=0, key=K)], BOTH, 0, "88 02 03 EF", 1007),
    ("an open text part cut inside a sequence", [frame(TEXT, b"a\xc3", fin=0, key=K)], BOTH, 0, "01 02 61 C3", 0),
    ("an open binary part", [frame(BIN, b"\xc3\x28", fin=0, key=K)], BOTH, 0, "02 02 C3 28", 0),
    ("a sequence completed by the next read", [frame(TEXT, b"a\xc3", fin=0, key=K), frame(CONT, b"\xa9", key=K)], BOTH, 0,
     "01 02 61 C3 80 01 A9", 0),
    ("a sequence broken by the next read", [frame(TEXT, b"a\xc3", fin=0, key=K), frame(CONT, b"\x28", key=K)], BOTH, 0,
     "01 02 61 C3 88 02 03 EF", 1007),
    # ---- the decode's error
    ("a continuation with none open, after a PING", [frame(PING, b"p", key=K) + frame(CONT, b"x", key=K)], BOTH, 0,
     "8A 01 70 88 02 03 EA", 1002),
    ("a text frame inside an open message", [frame(TEXT, b"ab", fin=0, key=K) + frame(TEXT, b"c", key=K)], BOTH, 0,
     "01 02 61 62 88 02 03 EA", 1002),
    ("RSV1", [frame(BIN, b"x", key=K, rsv=4)], BOTH, 0, "88 02 03 EA", 1002),
    ("opcode 3", [frame(3, b"x", key=K)], BOTH, 0, "88 02 03 EA", 1002),
    ("an unmasked frame", [frame(BIN, b"x", masked=False)], BOTH, 0, "88 02 03 EA", 1002),
    ("a PING without FIN", [frame(PING, b"x", fin=0, key=K)], BOTH, 0, "88 02 03 EA", 1002),
    ("a PING of 126 bytes", [frame(PING, bytes(126), key=K)], BOTH, 0, "88 02 03 EA", 1002),
    ("a frame over 2^32 bytes", [frame(BIN, b"y", key=K) + bytes.fromhex("82FF0000000100000001")], BOTH, 0,
     "82 01 79 88 02 03 F1", 1009),
    ("a protocol error with no flag set", [frame(PING, b"p", key=K) + frame(CONT, b"x", key=K)], 0, 0, "88 02 03 EA", 1002),
    # ---- what never fails
    ("a PING", [frame(PING, b"\xc3\x28", key=K)], BOTH, 0, "8A 02 C3 28", 0),
    ("a PONG", [frame(PONG, b"\xc3\x28", key=K)], BOTH, 0, "", 0),
    # ---- order
    ("a bad text, then a close", [frame(TEXT, b"\xff", key=K) + close(1000)], BOTH, 0, "88 02 03 EF", 1007),
    ("a close, then a bad text", [close(1000) + frame(TEXT, b"\xff", key=K)], BOTH, 0, "88 02 03 E8", 0),
    ("nothing after the failure", [frame(PING, b"", key=K) + frame(BIN, b"b", key=K) + frame(TEXT, b"\xff", key=K) +
                                   frame(PING, b"late", key=K)], BOTH, 0, "8A 00 82 01 62 88 02 03 EF", 1007),
    ("silence in the read after the failure", [frame(TEXT, b"\xff", key=K), frame(PING, b"late", key=K)], BOTH, 0,
     "88 02 03 EF", 1007),
]


def run_case(reads, flags, limit, make=StrictRef):
    flow, ref = FlowRef(), make(flags, limit) if make is StrictRef else make(flags)
    pending = b""
    for data in reads:
        out = flow.call(pending + data)
        pending = (pending + data)[out["res"]["resume_off"]:]
        ref.call(out)
    return ref


def test_the_case_list_names_every_code_and_every_non_failure():
    assert len({c[0] for c in CASES}) == len(CASES)
    assert {c[5] for c in CASES} == {0, 1002, 1007, 1009}
    assert close(1000) == CASES[0][1][0]              # the first case is spelled out byte by byte


def test_strictref_reproduces_the_case_list():
    for name, reads, flags, limit, want, code in CASES:
        ref = run_case(reads, flags, limit)
        assert ref.wire == bytes.fromhex(want), (name, ref.wire.hex())
        assert ref.state["fail_code"] == code, (name, ref.state)
        assert ref.state["close_sent"] == int(code != 0 or (bool(flags & CONTROL) and any(
            op == CLOSE for op, _, _ in ref.frames))), name
        if code:
            assert ref.frames[-1] == (CLOSE, 1, struct.pack(">H", code)), name


def test_close_code_is_the_code_received_only_when_a_close_failed():
    got = {name: run_case(reads, flags, limit).state for name, reads, flags, limit, _, _ in CASES}
    assert got["close 1005"]["close_code"] == 1005 and got["close of one byte"]["close_code"] == 1005
    assert got["reason C3"]["close_code"] == 1000 and got["close 1000"]["close_code"] == 1000
    assert got["text C3 28"]["close_code"] == 0 and got["RSV1"]["close_code"] == 0
    assert got["a bad text, then a close"]["close_code"] == 0


def test_every_close_code():
    allowed = set(range(1000, 1004)) | set(range(1007, 1015)) | set(range(3000, 5000))
    for c in range(65536):
        ok = c in allowed
        assert code_valid(c) == ok and _lib.close_code_valid(c) == ok, c
        assert close_failure(struct.pack(">H", c)) == (0 if ok else 1002), c
    for c in list(range(990, 1030)) + [2999, 3000, 4999, 5000, 65535]:
        ref = run_case([close(c)], BOTH, 0)
        assert ref.state["fail_code"] == (0 if c in allowed else 1002), c
        assert ref.frames == [(CLOSE, 1, struct.pack(">H", c if c in allowed else 1002))], c
    assert (_lib.FWS_CLOSE_PROTOCOL_ERROR, _lib.FWS_CLOSE_INVALID_DATA, _lib.FWS_CLOSE_TOO_BIG) == (1002, 1007, 1009)


def test_streams_with_no_failing_item_equal_replyref():
    """test_reply_cpu's random cut streams. Where no item fails every output of
    StrictRef is ReplyRef's; the streams that hold a TEXT message that is not
    UTF-8 are answered like ReplyRef up to it and then closed with 1007."""
    clean = failed = 0
    for seed in range(40):
        wire, _, _ = cc.random_stream(seed)
        rng = random.Random(9000 + seed)
        closing = [b"", struct.pack(">H", 1000), struct.pack(">H", 1001) + b"going away \xe2\x82\xac"][seed % 3]
        wire += cc.frame(cc.CLOSE, closing, key=cc.key(rng))
        wire += cc.frame(cc.BIN, b"after the close", key=cc.key(rng))
        fails = not all(ok for op, _, ok, _ in FlowRef().call(wire)["units"] if op == TEXT)
        clean, failed = clean + (not fails), failed + fails
        cuts = sorted({rng.randint(1, len(wire) - 1) for _ in range(rng.randint(3, 12))})
        for flags in (0, CONTROL, ECHO, BOTH):
            flow, a, b, pos = FlowRef(), ReplyRef(flags), StrictRef(flags), 0
            for end in cuts + [len(wire)]:
                out = flow.call(wire[pos:end])
                assert out["res"]["status"] == 0
                pos += out["res"]["resume_off"]
                x, y = a.call(out), b.call(out)
                if fails:
                    continue
                assert x["res"] == y["res"] and x["bytes"] == y["bytes"] and x["frames"] == y["frames"]
                assert x["records"].tobytes() == y["records"].tobytes()
                assert a.tx == b.tx and b.state == dict(a.state, fail_code=0)
            if fails:
                body = b.wire[:-4]
                assert b.wire[-4:] == bytes.fromhex("880203EF") and a.wire.startswith(body)
                assert len(a.wire) > len(body) or not flags & ECHO
                assert (b.state["close_sent"], b.state["fail_code"], b.state["close_code"]) == (1, 1007, 0)
            else:
                assert a.wire == b.wire
    assert clean >= 12 and failed >= 12


# ------------------------------------------------------------------ the ABI surface
def test_symbol_is_exported_and_bound():
    L = _lib.lib()
    assert hasattr(L, NAME) and NAME in _lib.exported_symbols()
    sig = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    assert sig[NAME][0] is C.c_int and len(sig[NAME][1]) == 20
    plain_args = list(sig[plain.NAME][1])
    assert list(sig[NAME][1]) == plain_args[:8] + [C.c_void_p, C.c_uint32, C.c_uint64] + plain_args[8:]
    assert callable(gpu.reply_messages_strict)
    src = open(HEADER).read()
    decl = re.search(r"int %s\((.*?)\);" % NAME, src, flags=re.S).group(1)
    assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == 20


def test_reply_state_keeps_its_16_bytes_and_gains_fail_code():
    src = open(HEADER).read()
    sizes = {k: int(v) for k, v in re.findall(r"\}\s*(fws_[a-z_]+);\s*/\*\s*(\d+) bytes", src)}
    assert sizes["fws_reply_state"] == _lib.REPLY_STATE.itemsize == 16
    decl = plain.struct_fields(src, "fws_reply_state")
    assert decl == [("close_sent", 4), ("close_code", 4), ("fail_code", 4), ("reserved", 4)]
    assert [d[0] for d in decl] == list(_lib.REPLY_STATE.names)
    assert [_lib.REPLY_STATE.fields[n][1] for n, _ in decl] == [0, 4, 8, 12]
    # the decode states the call reads, at the offsets the kernel uses
    assert (sizes["fws_msg_carry"], sizes["fws_msg_flow"]) == (_lib.MSG_CARRY.itemsize, _lib.MSG_FLOW.itemsize) == (64, 96)
    assert [_lib.MSG_CARRY.fields[k][1] for k in ("open_bytes", "utf8_bad", "prev_open_bytes")] == [8, 20, 32]
    assert _lib.MSG_FLOW.fields["frame_unread"][1] == 64


INDEX = {k: i for i, k in enumerate(("ctx", "reads", "n", "max_len", "msgs", "dst", "ctl", "mres", "cstates", "stride",
                                     "limit", "regions", "out", "frames", "res", "conns", "states", "n_conns", "flags",
                                     "stream"))}
POINTERS = ("ctx", "reads", "msgs", "dst", "ctl", "mres", "cstates", "regions", "out", "frames", "res", "conns", "states")


def stand_ins():
    """Pointers the checks must never follow: addresses inside one host page pair."""
    page = (C.c_uint8 * 8192)()
    base = (C.addressof(page) + 4095) & ~4095
    ok = [None] * 20
    for i, k in enumerate(POINTERS):
        ok[INDEX[k]] = base + 256 * i
    ok[INDEX["n"]], ok[INDEX["max_len"]], ok[INDEX["n_conns"]], ok[INDEX["flags"]] = 4, 4096, 4, BOTH
    ok[INDEX["stride"]], ok[INDEX["limit"]] = 96, 0
    return page, ok


def test_invalid_arguments_fail_before_any_device_call():
    f = getattr(_lib.lib(), NAME)
    page, ok = stand_ins()

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[INDEX[k]] = v
        return f(*a)

    for k in POINTERS:
        if k != "frames":                             # (optional: reaching the device call would follow ctx)
            assert call(**{k: None}) == _lib.FWS_ERR_INVALID, k
    for stride in (0, 32, 128, 63, 65, 95, 97, 0xFFFFFFFF):
        assert call(stride=stride) == _lib.FWS_ERR_INVALID, stride
    for stride in (64, 96):                           # (accepted: the next check is reached)
        assert call(stride=stride, out=None) == _lib.FWS_ERR_INVALID
    assert call(frames=None, out=None) == _lib.FWS_ERR_INVALID
    for misalign in (1, 4, 8):
        assert call(out=ok[INDEX["out"]] + misalign) == _lib.FWS_ERR_INVALID
    for max_len in (0, _lib.FWS_MSG_MULTI_MAX_READ + 1, 0xFFFFFFFF):
        assert call(max_len=max_len) == _lib.FWS_ERR_INVALID
    for flags in (4, 7, 8, 0x80000000, 0xFFFFFFFF):
        assert call(flags=flags) == _lib.FWS_ERR_INVALID
    for limit in (1, 1 << 63):                        # any limit is an argument, not an error
        assert call(limit=limit, out=None) == _lib.FWS_ERR_INVALID
    del page


def test_no_reads_is_no_launch():
    f = getattr(_lib.lib(), NAME)
    page, ok = stand_ins()
    a = list(ok)
    a[INDEX["n"]] = 0
    assert f(*a) == 0
    # nothing is looked at with n == 0, not even the arguments that would be refused
    assert f(None, None, 0, 0, *([None] * 5), 7, 0, *([None] * 6), 0, 0xFFFFFFFF, None) == 0
    del page
