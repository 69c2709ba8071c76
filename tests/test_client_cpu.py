"""CPU: the client role of the message path.

The ABI surface of fws_gpu_decode_messages_flow_client,
fws_gpu_reply_messages_multi_client and fws_gpu_reply_messages_strict_client --
the symbols, their signatures against the server calls', the argument checks
that come before any device call -- and the two predictors of client_ref.py
against the oracle's OnRecvData in the opposite role: ClientFlowRef delivers, for
server streams cut at random bytes, what orc.OrcSession(is_server=False) hands
out, and the masked reply wire the reply predictor builds is decoded by
orc.OrcSession(is_server=True) into the units the reply was asked to carry. No
device calls."""
import ctypes as C
import os
import random
import re

import client_ref as cr
import orc
import reply_ref as rr
import test_gpu_msg_carry as cc
import test_msg_flow_cpu as fc
from client_ref import BIN, CLOSE, PING, TEXT, ClientFlowRef, ClientReplyRef, ClientStrictRef, sframe
from flashws_amd import _lib, gpu
from msgflow_ref import feed
from reply_ref import CONTROL, ECHO

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fws_gpu.h")
DECODE = "fws_gpu_decode_messages_flow_client"
MULTI, STRICT = "fws_gpu_reply_messages_multi_client", "fws_gpu_reply_messages_strict_client"
INVALID = _lib.FWS_ERR_INVALID


# ------------------------------------------------------------------ 1. the ABI
def test_symbols_are_exported_and_bound():
    L = _lib.lib()
    sig = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    for name in (DECODE, MULTI, STRICT):
        assert hasattr(L, name) and name in _lib.exported_symbols(), name
        assert getattr(L, name).argtypes == sig[name][1] and sig[name][0] is C.c_int
    assert sig[DECODE] == sig["fws_gpu_decode_messages_flow"] and len(sig[DECODE][1]) == 14
    for client, server in ((MULTI, "fws_gpu_reply_messages_multi"), (STRICT, "fws_gpu_reply_messages_strict")):
        a, b = sig[client][1], sig[server][1]
        # one pointer more, between flags and stream
        assert len(a) == len(b) + 1 and a[:-2] == b[:-1] and a[-2] is C.c_void_p and a[-1] == b[-1], client
    for f in (gpu.decode_messages_flow_client, gpu.reply_messages_multi_client, gpu.reply_messages_strict_client):
        assert callable(f)


def test_the_header_declares_the_three_calls_and_drops_the_out_of_scope_remarks():
    src = open(HEADER).read()
    for name in (DECODE, MULTI, STRICT):
        assert re.search(r"\bint " + name + r"\(fws_gpu_ctx \*ctx,", src), name
    for name in (MULTI, STRICT):
        decl = re.search(r"\bint " + name + r"\((.*?)\);", src, flags=re.S).group(1)
        assert re.search(r"uint32_t flags,\s*const uint32_t \*dev_keys,\s*void \*stream$", decl), name
    assert "no client role yet" not in src
    # the flow decode and the two reply calls no longer rule the client out
    for name in ("fws_gpu_decode_messages_flow", "fws_gpu_reply_messages_multi", "fws_gpu_reply_messages_strict"):
        at = src.index("int " + name + "(")
        comment = src[src.rindex("/*", 0, at):at]
        scope = comment[comment.rindex("Out of scope"):]
        assert "client" not in scope and "masked" not in scope, name


def test_existing_structs_and_the_abi_version_did_not_move():
    fc.test_existing_structs_and_the_abi_version_did_not_move()
    fc.test_flow_state_is_96_bytes_in_the_header_order_with_msg_first()
    src = open(HEADER).read()
    sizes = {k: int(v) for k, v in re.findall(r"\}\s*(fws_[a-z_]+);\s*/\*\s*(\d+) bytes", src)}
    assert (sizes["fws_reply_state"], sizes["fws_reply_region"], sizes["fws_tx_result"]) == (16, 32, 32)
    assert (_lib.REPLY_STATE.itemsize, _lib.REPLY_REGION.itemsize, _lib.TX_RESULT.itemsize, _lib.TX_CONN.itemsize) == \
        (16, 32, 32, 32)


def test_decode_argument_checks_come_before_any_device_call():
    f = getattr(_lib.lib(), DECODE)
    page, ok = fc.stand_ins()

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[fc.INDEX[k]] = v
        return f(*a)

    for k in ("ctx", "wire", "reads", "frames", "msgs", "dst", "ctl", "res", "mres", "flows"):
        assert call(**{k: None}) == INVALID, k
    assert call(wire=ok[1] + 4) == INVALID
    assert call(dst=ok[7] + 8) == INVALID
    for max_len in (0, _lib.FWS_MSG_MULTI_MAX_READ + 1, 0xFFFFFFFF):
        assert call(max_len=max_len) == INVALID
    assert call(n=0) == 0
    assert f(*([None] * 3 + [0, 0] + [None] * 7 + [0, None])) == 0      # n == 0 looks at nothing
    del page


def reply_stand_ins(strict):
    """Pointers the checks must never follow, in the argument order of the two client reply calls."""
    page = (C.c_uint8 * 8192)()
    base = (C.addressof(page) + 4095) & ~4095
    p = [base + 256 * i for i in range(16)]
    names = ["ctx", "reads", "n", "max_len", "msgs", "dst", "ctl", "mres"]
    vals = [p[0], p[1], 4, 4096, p[2], p[3], p[4], p[5]]
    if strict:
        names += ["conn_states", "stride", "limit"]
        vals += [p[6], 96, 0]
    names += ["regions", "out", "frames", "res", "conns", "states", "n_conns", "flags", "keys", "stream"]
    vals += [p[7], p[8], p[9], p[10], p[11], p[12], 4, 3, p[13], None]
    return page, names, vals


def test_reply_argument_checks_come_before_any_device_call():
    for name, strict in ((MULTI, False), (STRICT, True)):
        f = getattr(_lib.lib(), name)
        page, names, ok = reply_stand_ins(strict)
        argtypes = {n: a for n, _, a in _lib.SIGNATURES}[name]
        assert len(ok) == len(argtypes)

        def call(**kw):
            a = list(ok)
            for k, v in kw.items():
                a[names.index(k)] = v
            return f(*a)

        assert call(keys=None) == INVALID, name
        pointers = ["ctx", "reads", "msgs", "dst", "ctl", "mres", "regions", "out", "res", "conns", "states"]
        for k in pointers + (["conn_states"] if strict else []):
            assert call(**{k: None}) == INVALID, (name, k)
        assert call(out=ok[names.index("out")] + 8) == INVALID
        for max_len in (0, _lib.FWS_MSG_MULTI_MAX_READ + 1, 0xFFFFFFFF):
            assert call(max_len=max_len) == INVALID
        for flags in (4, 8, 0x80000000):
            assert call(flags=flags) == INVALID
        if strict:
            for stride in (0, 32, 65, 128):
                assert call(stride=stride) == INVALID
        assert call(n=0) == 0
        assert call(n=0, keys=None) == 0
        assert f(*[None if t is C.c_void_p else 0 for t in argtypes]) == 0      # n == 0 looks at nothing
        del page


# ------------------------------------------------------------------ 2. the decode reference
def joined(out, parts, got):
    """A call's entries as units, the parts of a message joined (test_msg_flow_cpu's loop)."""
    for e in out["entries"]:
        if e["opcode"] >= 8:
            got.append((e["opcode"], out["ctl"][e["off"]:e["off"] + e["len"]]))
            continue
        body = out["dst"][e["off"]:e["off"] + e["len"]]
        if e["flags"] & _lib.FWS_MSG_CONTINUED:
            body = b"".join(parts) + body
        parts.clear()
        got.append((e["opcode"], body))
    if out["res"]["open_opcode"] and out["res"]["open_len"]:
        o = out["res"]["open_off"]
        parts.append(out["dst"][o:o + out["res"]["open_len"]])


def test_clientflowref_delivers_what_the_oracle_client_session_delivers():
    in_progress, lens = 0, set()
    for seed in range(40):
        wire, spans, units = cr.random_server_stream(seed)
        lens |= {f["plen"] for f in cr.client_parse(wire)[0]}
        cuts = cr.random_cuts(seed, wire, spans)
        session, ref = orc.OrcSession(is_server=False), ClientFlowRef()
        want, got, open_parts, parts, pong_parts = [], [], [], [], []
        pos = last = 0
        for b in cuts + [len(wire)]:
            fc.session_units(session, wire[last:b], open_parts, want, pong_parts)
            last = b
            while True:                               # (a read of many short frames: the header limit)
                out = ref.call(wire[pos:b])
                assert out["res"]["status"] in (0, _lib.FWS_ERR_CAPACITY), seed
                pos += out["res"]["resume_off"]
                joined(out, parts, got)
                if out["res"]["status"] == 0:
                    break
            assert b - pos < 10 + 125
            assert got == want[:len(got)], (seed, b)
            st = ref.state
            assert st["frame_key"] == 0
            if st["frame_unread"]:                    # the read ended inside a data frame
                head = session.head()
                assert head.unread_pl_len == st["frame_unread"], (seed, b)
                assert head.last_rx_fin_flag == st["frame_fin"] and pos == b
                in_progress += 1
        assert got == want == units and pos == len(wire), seed
        assert [(u[0], u[1]) for u in cr.whole(wire)[0]] == units, seed
    assert in_progress > 40 and set(cr.EDGES) <= lens


def test_clientflowref_delivers_the_same_units_for_every_cut():
    stream = cr.twelve_frames()
    units, status = cr.whole(stream)
    assert status == 0 and len(units) == 8
    # the server role's twelve frames: the same opcodes, lengths, verdicts and fragment counts
    assert [(u[0], len(u[1]), u[2], u[3]) for u in units] == \
        [(u[0], len(u[1]), u[2], u[3]) for u in cc.whole(cc.twelve_frames())[0]]
    for cut in range(len(stream) + 1):
        ref = ClientFlowRef()
        got, calls = feed(ref, stream, [cut])
        assert got == units and ref.state["msg"]["wire_bytes"] == len(stream), cut
        assert ref.state["frame_unread"] == 0 and ref.state["msg"]["n_msgs"] == 8 and ref.state["frame_key"] == 0


def test_a_masked_frame_is_refused_by_both_the_walk_and_the_oracle():
    ok = sframe(BIN, b"fine") + sframe(PING, b"p")
    masked = cc.frame(TEXT, b"from a client", key=0x01020304)
    wire = ok + masked + ok
    out = ClientFlowRef().call(wire)
    assert out["res"]["status"] == out["dres"]["status"] == _lib.FWS_ERR_MASKED
    assert out["dres"]["err_off"] == out["dres"]["consumed"] == len(ok) and out["res"]["resume_off"] == len(ok)
    assert [(u[0], u[1]) for u in out["units"]] == [(BIN, b"fine"), (PING, b"p")]
    session = orc.OrcSession(is_server=False)
    assert session.feed(wire)[0] == _lib.FWS_ERR_MASKED
    # the parse alone: the roles mirror each other
    assert cc.ref_parse(ok)[1] == _lib.FWS_ERR_NOT_MASKED and cr.client_parse(masked)[1] == _lib.FWS_ERR_MASKED


# ------------------------------------------------------------------ 3. the reply reference
def server_units(wire):
    """The masked wire through the oracle's server-role OnRecvData: (units, the open message's parts)."""
    session, units, open_parts, pong_parts = orc.OrcSession(is_server=True), [], [], []
    fc.session_units(session, wire, open_parts, units, pong_parts)
    return units, b"".join(open_parts)


def test_masked_replies_are_decoded_by_the_oracle_server_into_what_was_asked():
    frames = 0
    for seed in range(40):
        wire, spans, _ = cr.random_server_stream(seed)
        wire += sframe(CLOSE, b"\x03\xe8done") + sframe(TEXT, b"late")
        cuts = cr.random_cuts(seed, wire, spans)
        rng = random.Random(seed)
        flow, reply = ClientFlowRef(), ClientReplyRef(CONTROL | ECHO)
        pos, keys = 0, []
        for b in cuts + [len(wire)]:
            while True:
                out = flow.call(wire[pos:b])
                pos += out["res"]["resume_off"]
                reply.key = rng.getrandbits(32)
                got = reply.call(out)
                keys += [_lib.FWS_TX_FRAG_KEY(reply.key, j) for j in range(got["res"]["n_frames"])]
                assert [int(k) for k in got["records"]["key"]] == keys[len(keys) - got["res"]["n_frames"]:]
                if out["res"]["status"] == 0:
                    break
        walked = cr.walk_client_frames(reply.wire)
        assert [(op, fin, p) for op, fin, p, _ in walked] == reply.frames and [k for *_, k in walked] == keys
        asked, still_open = rr.messages(reply.frames)
        got, open_bytes = server_units(reply.wire)
        assert got == asked and asked[-1] == (CLOSE, b"\x03\xe8done"), seed
        assert open_bytes == (still_open[1] if still_open else b"")
        assert reply.state["close_sent"] == 1 and reply.state["close_code"] == 1000
        frames += len(walked)
    assert frames > 1000


def test_the_failing_close_is_eight_masked_bytes():
    bad = sframe(TEXT, b"ok") + sframe(TEXT, b"\xff") + sframe(BIN, b"never")
    for flags in range(4):
        flow, reply = ClientFlowRef(), ClientStrictRef(flags)
        reply.key = 0xA1B2C3D4
        got = reply.call(flow.call(bad))
        j = 1 if flags & ECHO else 0
        k = _lib.FWS_TX_FRAG_KEY(reply.key, j).to_bytes(4, "little")
        tail = bytes([0x88, 0x82]) + k + bytes(a ^ b for a, b in zip(b"\x03\xef", k))
        assert got["bytes"][-8:] == tail and got["res"]["n_frames"] == j + 1 and reply.state["fail_code"] == 1007
        assert got["res"]["out_len"] == (8 if flags & ECHO else 0) + 8
        assert server_units(got["bytes"])[0][-1] == (CLOSE, b"\x03\xef")
