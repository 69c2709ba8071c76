"""CPU: the ABI surface of fws_gpu_reply_messages_multi -- the symbol, the two
new structs against the header and the numpy mirrors, the argument checks that
come before any device call -- and ReplyRef (reply_ref.py), the GPU tests'
predictor, against the oracle's OnRecvData: for random streams cut at random
bytes its PONGs and its CLOSE carry what the session's PONG_SENT and
CLOSE_RECV events carry, its echo parses back into the session's messages, and
the reply stream is sequence-valid. No device calls."""
import ctypes as C
import os
import random
import re
import struct

import orc
import test_gpu_msg_carry as cc
from flashws_amd import _lib, gpu
from msgflow_ref import FlowRef
from reply_ref import CONTROL, ECHO, ReplyRef, messages, walk_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fws_gpu.h")
NAME = "fws_gpu_reply_messages_multi"


def test_symbol_is_exported_and_bound():
    L = _lib.lib()
    assert hasattr(L, NAME)
    assert NAME in _lib.exported_symbols()
    sig = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    assert sig[NAME][0] is C.c_int and len(sig[NAME][1]) == 17
    assert [a for a in sig[NAME][1] if a is C.c_uint32] == [C.c_uint32] * 4     # n, max_len, n_conns, flags
    assert callable(gpu.reply_messages_multi) and callable(gpu.read_reply_state) and callable(gpu.MessageResponder)
    assert (_lib.FWS_REPLY_CONTROL, _lib.FWS_REPLY_ECHO) == (1, 2)


def struct_fields(src, name):
    body = re.search(r"typedef struct %s \{(.*?)\}" % name, src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for typ, names in re.findall(r"\b(u?int\d+_t)\s+([a-z0-9_, ]+);", body):
        out += [(n.strip(), int(re.search(r"\d+", typ).group()) // 8) for n in names.split(",")]
    return out


def test_the_two_structs_are_16_and_32_bytes_in_the_header_order():
    src = open(HEADER).read()
    sizes = {k: int(v) for k, v in re.findall(r"\}\s*(fws_[a-z_]+);\s*/\*\s*(\d+) bytes", src)}
    assert sizes["fws_reply_state"] == _lib.REPLY_STATE.itemsize == 16
    assert sizes["fws_reply_region"] == _lib.REPLY_REGION.itemsize == 32
    for name, dt in (("fws_reply_state", _lib.REPLY_STATE), ("fws_reply_region", _lib.REPLY_REGION)):
        decl = struct_fields(src, name)
        assert [d[0] for d in decl] == list(dt.names), name
        off = 0
        for field, width in decl:
            assert dt.fields[field][1] == off and dt.fields[field][0].itemsize == width, (name, field)
            off += width
        assert off == dt.itemsize
    assert re.search(r"#define\s+FWS_REPLY_CONTROL\s+1u", src) and re.search(r"#define\s+FWS_REPLY_ECHO\s+2u", src)


def test_existing_structs_and_the_abi_version_did_not_move():
    src = open(HEADER).read()
    sizes = {k: int(v) for k, v in re.findall(r"\}\s*(fws_[a-z_]+);\s*/\*\s*(\d+) bytes", src)}
    assert (sizes["fws_frame_desc"], sizes["fws_frame_info"], sizes["fws_decode_result"]) == (24, 24, 40)
    assert (sizes["fws_msg_info"], sizes["fws_msg_result"], sizes["fws_msg_carry"], sizes["fws_msg_read"],
            sizes["fws_msg_flow"]) == (32, 64, 64, 64, 96)
    assert (sizes["fws_tx_desc"], sizes["fws_tx_conn"], sizes["fws_tx_send"], sizes["fws_tx_result"]) == \
        (24, 32, 64, 32)
    assert (_lib.TX_CONN.itemsize, _lib.TX_SEND.itemsize, _lib.TX_RESULT.itemsize) == (32, 64, 32)
    assert (_lib.MSG_INFO.itemsize, _lib.MSG_RESULT.itemsize, _lib.MSG_READ.itemsize, _lib.MSG_FLOW.itemsize) == \
        (32, 64, 64, 96)
    assert re.search(r"#define\s+FWS_GPU_ABI_VERSION\s+1\b", src)
    assert _lib.lib().fws_gpu_abi_version() == 1


INDEX = {k: i for i, k in enumerate(("ctx", "reads", "n", "max_len", "msgs", "dst", "ctl", "mres", "regions", "out",
                                     "frames", "res", "conns", "states", "n_conns", "flags", "stream"))}
POINTERS = ("ctx", "reads", "msgs", "dst", "ctl", "mres", "regions", "out", "frames", "res", "conns", "states")


def stand_ins():
    """Pointers the checks must never follow: addresses inside one host page pair."""
    page = (C.c_uint8 * 8192)()
    base = (C.addressof(page) + 4095) & ~4095
    ok = [None] * 17
    for i, k in enumerate(POINTERS):
        ok[INDEX[k]] = base + 256 * i
    ok[INDEX["n"]], ok[INDEX["max_len"]], ok[INDEX["n_conns"]], ok[INDEX["flags"]] = 4, 4096, 4, CONTROL | ECHO
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
    assert call(frames=None, out=None) == _lib.FWS_ERR_INVALID
    for misalign in (1, 4, 8):
        assert call(out=ok[INDEX["out"]] + misalign) == _lib.FWS_ERR_INVALID
    for max_len in (0, _lib.FWS_MSG_MULTI_MAX_READ + 1, 0xFFFFFFFF):
        assert call(max_len=max_len) == _lib.FWS_ERR_INVALID
    for flags in (4, 7, 8, 0x80000000, 0xFFFFFFFF):
        assert call(flags=flags) == _lib.FWS_ERR_INVALID
    del page


def test_no_reads_is_no_launch():
    f = getattr(_lib.lib(), NAME)
    page, ok = stand_ins()
    a = list(ok)
    a[INDEX["n"]] = 0
    assert f(*a) == 0
    # nothing is looked at with n == 0, not even the arguments that would be refused
    assert f(None, None, 0, 0, *([None] * 10), 0, 0xFFFFFFFF, None) == 0
    del page


# ------------------------------------------------------------------ ReplyRef against OnRecvData
def close_payload(seed, rng):
    return [b"", b"\x03", struct.pack(">H", 1000), struct.pack(">H", 1001) + cc.payload(rng, seed % 120)][seed % 4]


def session_replies(session, data, state):
    """One read through the oracle's OnRecvData: the PONG_SENT payloads, the
    CLOSE_RECV (payload, code) and the data messages completed, up to the CLOSE."""
    ret, buf, ev, ctl = session.feed(data)
    assert ret == 0
    for e in ev:
        if state["close"] is not None:
            return
        kind, o, n = int(e["kind"]), int(e["ctl_off"]), int(e["size"])
        if kind == 1:
            state["pongs"].append(ctl[o:o + n].tobytes())
        elif kind == 2:
            state["close"] = (ctl[o:o + n].tobytes(), int(e["key"]))
        elif kind == 0 and not e["is_ctl"]:
            d = int(e["data_off"])
            state["parts"].append(buf[d:d + n].tobytes())
            if e["msg_end"]:
                state["msgs"].append((int(e["opcode"]), b"".join(state["parts"])))
                state["parts"] = []


def test_replyref_answers_what_the_oracle_session_answers():
    pings = parts_echoed = 0
    for seed in range(40):
        wire, _, _ = cc.random_stream(seed)
        rng = random.Random(9000 + seed)
        closing = close_payload(seed, rng)
        wire += cc.frame(cc.CLOSE, closing, key=cc.key(rng)) + cc.frame(cc.BIN, b"after the close", key=cc.key(rng))
        cuts = sorted({rng.randint(1, len(wire) - 1) for _ in range(rng.randint(3, 12))})
        session = orc.OrcSession(is_server=True)
        want = dict(pongs=[], close=None, msgs=[], parts=[])
        refs = {flags: (FlowRef(), ReplyRef(flags)) for flags in (0, CONTROL, ECHO, CONTROL | ECHO)}
        pos = dict.fromkeys(refs, 0)
        last = 0
        for b in cuts + [len(wire)]:
            session_replies(session, wire[last:b], want)
            last = b
            for flags, (flow, reply) in refs.items():
                out = flow.call(wire[pos[flags]:b])
                assert out["res"]["status"] == 0
                pos[flags] += out["res"]["resume_off"]
                got = reply.call(out)
                assert got["res"]["status"] == 0 and reply.wire.endswith(got["bytes"])
                parts_echoed += int(flags == ECHO and out["res"]["open_len"] > 0)
        assert want["close"] == (closing, 1005 if len(closing) < 2 else int.from_bytes(closing[:2], "big"))
        pings += len(want["pongs"])
        for flags, (flow, reply) in refs.items():
            frames = walk_frames(reply.wire)
            assert frames == reply.frames
            units, still_open = messages(frames)      # asserts the sequencing, and that nothing follows a CLOSE
            pongs = [p for op, p in units if op == cc.PONG]
            closes = [p for op, p in units if op == cc.CLOSE]
            data = [(op, p) for op, p in units if op < 8]
            if flags & CONTROL:
                assert pongs == want["pongs"] and closes == [want["close"][0]], (seed, flags)
                assert (reply.state["close_sent"], reply.state["close_code"]) == (1, want["close"][1])
                assert still_open is None
            else:
                assert not pongs and not closes and reply.state == dict(close_sent=0, close_code=0, reserved=0)
            if flags & ECHO:
                # without FWS_REPLY_CONTROL the message behind the CLOSE is echoed as well
                extra = [] if flags & CONTROL else [(cc.BIN, b"after the close")]
                assert data == want["msgs"] + extra, (seed, flags)
            else:
                assert not data
            assert reply.tx["frames"] == len(frames) and reply.tx["wire_bytes"] == len(reply.wire)
            assert reply.tx["last_msg_not_fin"] == 0
    assert pings > 40 and parts_echoed > 40


def test_replyref_parts_are_continuations_and_a_ping_goes_between_them():
    rng = random.Random(5)
    body = cc.payload(rng, 40)
    wire = (cc.frame(cc.BIN, body[:10], fin=0, key=cc.key(rng)) + cc.frame(cc.PING, b"hi", key=cc.key(rng)) +
            cc.frame(cc.CONT, body[10:], fin=1, key=cc.key(rng)))
    whole = ReplyRef(CONTROL | ECHO)
    whole.call(FlowRef().call(wire))
    # a message that arrives whole is one entry: the PING's answer comes first, then one frame
    assert whole.frames == [(cc.PONG, 1, b"hi"), (cc.BIN, 1, body)]
    flow, cut = FlowRef(), ReplyRef(CONTROL | ECHO)
    a = cut.call(flow.call(wire[:9]))                 # 3 of the first fragment's 10 bytes
    assert a["frames"] == [(cc.BIN, 0, body[:3])] and cut.tx["last_msg_not_fin"] == 1
    b = cut.call(flow.call(wire[9:]))
    assert b["frames"] == [(cc.PONG, 1, b"hi"), (0, 1, body[3:])] and cut.tx["last_msg_not_fin"] == 0
    assert messages(walk_frames(cut.wire))[0] == [(cc.PONG, b"hi"), (cc.BIN, body)]
    # an open part of 0 bytes gives no frame: the completing frame carries the opcode
    flow, empty = FlowRef(), ReplyRef(ECHO)
    assert empty.call(flow.call(wire[:6]))["frames"] == [] and empty.tx["last_msg_not_fin"] == 0
    assert empty.call(flow.call(wire[6:]))["frames"] == [(cc.BIN, 1, body)]
