"""GPU parity of the client role: fws_gpu_decode_messages_flow_client against
ClientFlowRef and fws_gpu_reply_messages_multi_client / _strict_client against
the client reply predictors (client_ref.py; test_client_cpu.py holds them
against the oracle's OnRecvData in the opposite role).

The harness is the server role's: a decode call in Multi's arena
(test_gpu_msg_flow.Flow) and a reply call in a sentinel-filled arena
(test_gpu_reply.Reply), both compared whole -- every region, record, result
and state exactly, every other byte the sentinel or the input. Only the launch,
the predictor and the sizes that depend on the header length differ. All
comparisons are exact."""
import gzip
import hashlib
import json
import os
import random
import struct

import numpy as np
import pytest
import torch

import client_ref as cr
import orc
import reply_ref as rr
import test_gpu_msg_carry as cc
import test_gpu_msg_flow as fm
import test_gpu_msg_multi as mm
import test_gpu_reply as rp
import txmulti_ref as tr
from client_ref import (BIN, CLOSE, CONT, PING, PONG, TEXT, ClientFlowRef, ClientReplyRef, ClientStrictRef, sframe,
                        walk_client_frames)
from flashws_amd import _lib, gpu
from reply_ref import CONTROL, ECHO, messages, walk_frames
from test_gpu_msg_carry import FILL, GUARD, NONE, frame, key

pytestmark = pytest.mark.gpu

CAPACITY, DECLINED, INVALID, MASKED = (_lib.FWS_ERR_CAPACITY, _lib.FWS_ERR_DECLINED, _lib.FWS_ERR_INVALID,
                                       _lib.FWS_ERR_MASKED)
SMALL, FULL, BOTH, FORMS = rp.SMALL, rp.FULL, rp.BOTH, rp.FORMS
FRAG_KEY = _lib.FWS_TX_FRAG_KEY
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tx_cases.json.gz")


# ------------------------------------------------------------------ the harness
class Conns(fm.Conns):
    """fm.Conns whose references are ClientFlowRef."""

    def __init__(self, cuda, n):
        super().__init__(cuda, n)
        self.ref = [ClientFlowRef() for _ in range(n)]


class Flow(fm.Flow):
    """fm.Flow launched as the client call; a frame slice sized for 2-byte frames."""

    def __init__(self, cuda, conns, reads, max_len=None):
        for r in reads:
            r.setdefault("cap", len(r["wire"]) // 2 + 16)
        super().__init__(cuda, conns, reads, max_len)

    def launch(self, ctx, stream=None):
        rc = gpu.decode_messages_flow_client(ctx, self.arena, self.t("reads"), self.n, self.max_len, self.t("frames"),
                                             self.t("msgs"), self.arena, self.arena, self.t("res"), self.t("mres"),
                                             self.conns.t, self.conns.n_dev, stream=stream)
        assert rc == 0, rc


def run(ctx, cuda, conns, reads, max_len=None):
    """One client decode call, checked in full: (the references' outputs, the call, the states' bytes)."""
    m = Flow(cuda, conns, reads, max_len)
    outs = m.expect()
    m.launch(ctx)
    m.check()
    return outs, m, conns.check()


def feed_all(ctx, cuda, conns, streams, cuts, max_len=None, **caps):
    """fm.feed_all over the client call."""
    n = len(streams)
    ends = [sorted(set(cs)) + [len(s)] for s, cs in zip(streams, cuts)]
    pos, calls = [0] * n, []
    for k in range(max(map(len, ends))):
        reads = [dict(wire=streams[c][pos[c]:ends[c][min(k, len(ends[c]) - 1)]], conn=c, **caps) for c in range(n)]
        outs, _, _ = run(ctx, cuda, conns, reads, max_len)
        for c, out in enumerate(outs):
            pos[c] += out["res"]["resume_off"]
        calls.append(outs)
    return calls


def plain(units):
    return [(op, body) for op, body, *_ in units]


class RConns(rp.RConns):
    """rp.RConns for a client: the references build masked frames (strict: ClientStrictRef with the calls' limit)."""

    def __init__(self, cuda, n, flags=BOTH, strict=False, limit=0):
        super().__init__(cuda, n, flags)
        self.strict, self.limit = strict, limit
        self.ref = [ClientStrictRef(flags, limit) if strict else ClientReplyRef(flags) for _ in range(n)]


class Reply(rp.Reply):
    """rp.Reply launched as one of the client calls. keys[i] is read i's key, in a
    device array with a guard behind it; a region is sized for 14-byte headers
    and the 8-byte failing CLOSE."""

    def __init__(self, cuda, m, rc, keys, opts=None, flags=None):
        opts = [dict(o) for o in (opts or [{} for _ in range(m.n)])]
        for r, o in zip(m.reads, opts):
            o.setdefault("out_cap", len(r["wire"]) + 14 * (r["msg_cap"] + 1) + 8 + 16)
        super().__init__(cuda, m, rc, opts, flags)
        assert len(keys) == m.n
        self.keys = [k & 0xFFFFFFFF for k in keys]
        host = np.full(4 * m.n + GUARD, FILL, dtype=np.uint8)
        host[:4 * m.n] = np.array(self.keys, dtype="<u4").view(np.uint8)
        self.keys_in = host
        self.kt = torch.from_numpy(host).to(cuda)

    def expect(self):
        for r, k in zip(self.m.reads, self.keys):
            self.rc.ref[r["conn"]].key = k
        return super().expect()

    def launch(self, ctx, stream=None):
        m, c = self.m, self.rc
        if c.strict:
            rc = gpu.reply_messages_strict_client(ctx, m.t("reads"), m.n, m.max_len, m.t("msgs"), m.arena, m.arena,
                                                  m.t("mres"), m.conns.t, fm.SSZ, c.limit, self.t("regions"),
                                                  self.arena, self.t("frames"), self.t("res"), c.tx, c.st, c.n_dev,
                                                  self.flags, self.kt, stream=stream)
        else:
            rc = gpu.reply_messages_multi_client(ctx, m.t("reads"), m.n, m.max_len, m.t("msgs"), m.arena, m.arena,
                                                 m.t("mres"), self.t("regions"), self.arena, self.t("frames"),
                                                 self.t("res"), c.tx, c.st, c.n_dev, self.flags, self.kt,
                                                 stream=stream)
        assert rc == 0, rc

    def check(self):
        super().check()
        assert self.kt.cpu().numpy().tobytes() == self.keys_in.tobytes(), "the keys were modified"


def reply(ctx, cuda, m, rc, keys, opts=None, flags=None):
    r = Reply(cuda, m, rc, keys, opts, flags)
    r.expect()
    r.launch(ctx)
    torch.cuda.synchronize()
    r.check()
    rc.check()
    m.conns.check()                                   # the decode's states: read, never written
    return r


def step(ctx, cuda, conns, rc, reads, keys, max_len=None, opts=None):
    """client decode + client reply, both checked in full: (the decode's outputs, the reply call)."""
    outs, m, _ = run(ctx, cuda, conns, reads, max_len)
    return outs, reply(ctx, cuda, m, rc, keys, opts)


def some_keys(rng, n):
    """0, all ones and random keys."""
    return [(0, 0xFFFFFFFF)[i] if i < 2 else rng.getrandbits(32) for i in range(n)]


# ------------------------------------------------------------------ 4. the client decode
@FORMS
def test_every_cut_at_once(ctx, cuda, max_len):
    stream = cr.twelve_frames()
    L = len(stream)
    units, status = cr.whole(stream)
    assert status == 0 and len(units) == 8
    conns = Conns(cuda, L + 1)
    calls = feed_all(ctx, cuda, conns, [stream] * (L + 1), [[c] for c in range(L + 1)], max_len)
    in_frame = sum(1 for o in calls[0] if o["state"]["frame_unread"])
    leads = sum(1 for o in calls[1] for e in o["entries"] if e["flags"] and e["first_frame"] == NONE)
    assert in_frame > 30 and leads > 10
    for c in range(L + 1):
        assert conns.units[c] == units, c
        st = conns.ref[c].state
        assert st["msg"]["wire_bytes"] == L and st["frame_unread"] == st["frame_key"] == 0
        assert calls[-1][c]["res"]["status"] == 0


@FORMS
def test_random_streams_many_connections_per_launch(ctx, cuda, max_len):
    made = [cr.random_server_stream(seed, edges=(0, 125, 126)) for seed in range(20)]
    streams = [w for w, _, _ in made]
    cuts = [cr.random_cuts(seed, w, spans, 2, 6) for seed, (w, spans, _) in enumerate(made)]
    assert max(map(len, streams)) <= SMALL
    conns = Conns(cuda, 20)
    calls = feed_all(ctx, cuda, conns, streams, cuts, max_len)
    assert sum(1 for outs in calls for o in outs if o["state"]["frame_unread"]) >= 10
    for c, (w, _, units) in enumerate(made):
        assert plain(conns.units[c]) == units and conns.ref[c].state["msg"]["wire_bytes"] == len(w), c


def test_header_forms_at_their_boundaries(ctx, cuda):
    rng = random.Random(41)
    sizes = (0, 1, 125, 126, 127, 65535, 65536, 65537)
    bodies = [cc.payload(rng, n) for n in sizes]
    streams = [sframe(BIN, b) + sframe(TEXT, b"after") for b in bodies]
    hdr = [2, 2, 2, 4, 4, 4, 10, 10]
    # whole; cut at byte 3 (inside the longer headers); cut in the middle of the payload
    for cuts in ([[] for _ in sizes], [[3] for _ in sizes], [[h + n // 2] for h, n in zip(hdr, sizes)]):
        conns = Conns(cuda, len(sizes))
        calls = feed_all(ctx, cuda, conns, streams, cuts)
        for c, b in enumerate(bodies):
            assert plain(conns.units[c]) == [(BIN, b), (TEXT, b"after")], (c, cuts[c])
        if not cuts[0]:
            recs = [np.frombuffer(o["frames"], dtype=_lib.FRAME_INFO) for o in calls[0]]
            assert [int(r[0]["hdr_len"]) for r in recs] == hdr and all(int(r[0]["key"]) == 0 for r in recs)
        elif cuts[0] == [3]:                          # a partial header waits (the empty frame: the next one's)
            assert [o["dres"]["carry_hdr_len"] for o in calls[0]] == [1, 0, 0, 3, 3, 3, 3, 3]


def test_a_300_kib_frame_in_16_kib_reads(ctx, cuda):
    rng = random.Random(42)
    body = cc.random_text(rng, 300 << 10)
    bad = bytearray(body)
    at = next(i for i in range(200000, 300000) if bad[i] >= 0xE0)
    bad[at + 1] = 0x28                                # a lead byte followed by '('
    streams = [sframe(TEXT, x) + sframe(PING, b"behind") for x in (body, bytes(bad))]
    assert len(streams[0]) == (300 << 10) + 10 + 8
    step_ = (16 << 10) - 144
    cuts = [list(range(step_, len(s), step_)) for s in streams]
    conns = Conns(cuda, 2)
    calls = feed_all(ctx, cuda, conns, streams, cuts, SMALL)
    assert sum(1 for outs in calls for o in outs if o["dres"]["n_frames"] == 0 and o["res"]["data_bytes"]) >= 30
    assert conns.units[0] == [(TEXT, body, 1, 1), (PING, b"behind", 0, 1)]
    assert conns.units[1] == [(TEXT, bytes(bad), 0, 1), (PING, b"behind", 0, 1)]
    assert calls[0][0]["state"]["frame_len"] == 300 << 10 and calls[0][0]["state"]["frame_key"] == 0


@FORMS
@pytest.mark.parametrize("count", [257, 300])
def test_more_two_byte_frames_than_one_call_takes(ctx, cuda, max_len, count):
    ops = [(BIN, 0), (CONT, 0), (PING, 1), (CONT, 1), (TEXT, 1), (PONG, 1)]
    stream = b"".join(sframe(op, b"", fin=fin) for op, fin in (ops[j % 6] for j in range(count)))
    assert len(stream) == 2 * count
    units, status = cr.whole(stream)                  # (the walk's own first call stops at header 257 as well)
    assert status == CAPACITY
    conns = Conns(cuda, 1)
    outs, _, _ = run(ctx, cuda, conns, [dict(wire=stream, conn=0)], max_len)
    r, d = outs[0]["res"], outs[0]["dres"]
    assert (r["status"], r["resume_off"], d["status"], d["n_frames"], d["consumed"]) == (CAPACITY, 512, CAPACITY, 257, 512)
    outs, _, _ = run(ctx, cuda, conns, [dict(wire=stream[512:], conn=0)], max_len)
    assert outs[0]["res"]["status"] == 0 and outs[0]["dres"]["n_frames"] == count - 256
    unit_of = {2: PING, 3: BIN, 4: TEXT, 5: PONG}     # (the FIN continuation completes the BIN message)
    want = [(unit_of[j % 6], b"") for j in range(count) if j % 6 in unit_of]
    assert plain(conns.units[0]) == want and conns.ref[0].state["msg"]["wire_bytes"] == 2 * count


@FORMS
def test_utf8_sequence_cut_by_a_read(ctx, cuda, max_len):
    streams, cuts, want = [], [], []
    for seq in cc.VALID + cc.ILL_FORMED:
        ok = int(seq in cc.VALID)
        for pre, post in ((b"", b""), (b"ab", b"cd"), (b"", b"cd"), (b"ab", b"")):
            body = pre + seq + post
            for at in range(len(seq) + 1):            # the cut before byte `at` of the sequence
                # inside one frame
                streams.append(sframe(TEXT, body))
                cuts.append([2 + len(pre) + at])
                want.append([(TEXT, body, ok, 1)])
                # across two frames, the read cut at the seam
                k = len(pre) + at
                first = sframe(TEXT, body[:k], fin=0)
                streams.append(first + sframe(CONT, body[k:], fin=1))
                cuts.append([len(first)])
                want.append([(TEXT, body, ok, 2)])
    conns = Conns(cuda, len(streams))
    calls = feed_all(ctx, cuda, conns, streams, cuts, max_len)
    assert sum(1 for o in calls[0] if o["state"]["frame_unread"]) > len(streams) // 4
    assert any(o["state"]["msg"]["utf8_bad"] for o in calls[0])
    for c in range(len(streams)):
        assert conns.units[c] == want[c], (c, streams[c], cuts[c])


def test_capacity_refusals_leave_the_state_untouched(ctx, cuda):
    rng = random.Random(43)
    text = cc.random_text(rng, 60)
    opener = sframe(TEXT, text)
    cut = len(opener) - 25
    tail = opener[cut:] + sframe(PING, b"ping!") + sframe(BIN, b"more")
    conns = Conns(cuda, 5)
    run(ctx, cuda, conns, [dict(wire=opener[:cut], conn=c) for c in range(5)])
    assert all(r.state["frame_unread"] == 25 for r in conns.ref)
    short = {1: dict(dst_cap=28), 2: dict(ctl_cap=4), 3: dict(msg_cap=2), 4: dict(dst_cap=16)}
    before = conns.check()
    outs, _, after = run(ctx, cuda, conns, [dict(wire=tail, conn=c, **short.get(c, {})) for c in range(5)])
    for c in (1, 2, 3, 4):
        r = outs[c]["res"]
        assert (r["status"], r["resume_off"], r["n_msgs"], r["data_bytes"], r["ctl_bytes"]) == (CAPACITY, 0, 3, 29, 5)
        assert after[c] == before[c] and (outs[c]["dst"], outs[c]["ctl"]) == (b"", b"")
    assert outs[0]["res"]["status"] == 0
    run(ctx, cuda, conns, [dict(wire=b"" if c == 0 else tail, conn=c, dst_cap=32, ctl_cap=5, msg_cap=3)
                           for c in range(5)])
    for c in range(5):
        assert plain(conns.units[c]) == [(TEXT, text), (PING, b"ping!"), (BIN, b"more")], c


def test_an_error_stays_on_its_connection(ctx, cuda):
    made = [cr.random_server_stream(seed, edges=(0, 125, 126)) for seed in range(16)]
    streams = [(w, cr.random_cuts(seed, w, spans, 2, 4)) for seed, (w, spans, _) in enumerate(made)]
    bad_opcode = bytes([0x83, 0x00])

    def both_calls(with_error):
        conns = Conns(cuda, 16)
        firsts = [w[:cs[0]] for w, cs in streams]
        one = run(ctx, cuda, conns, [dict(wire=w, conn=c) for c, w in enumerate(firsts)])
        seconds = [w[cs[0] - (len(firsts[c]) - one[0][c]["res"]["resume_off"]):] for c, (w, cs) in enumerate(streams)]
        if with_error:                                # behind what is left of a frame in progress
            lead = conns.ref[7].state["frame_unread"]
            seconds[7] = seconds[7][:lead] + bad_opcode + seconds[7][lead:]
        return one, run(ctx, cuda, conns, [dict(wire=w, conn=c) for c, w in enumerate(seconds)])

    clean, dirty = both_calls(False), both_calls(True)
    assert dirty[1][0][7]["res"]["status"] == _lib.FWS_ERR_OPCODE and clean[1][0][7]["res"]["status"] == 0
    for (_, a, sa), (_, b, sb) in zip(clean, dirty):
        for c in range(16):
            if c == 7:
                continue
            for k in ("dst", "ctl", "frames", "msgs"):
                assert a.region(a.got, a.reads[c], k) == b.region(b.got, b.reads[c], k), (c, k)
            for k, sz in (("res", mm.DSZ), ("mres", mm.RSZ)):
                o = a.sec[k][0] + c * sz
                assert a.got[o:o + sz].tobytes() == b.got[b.sec[k][0] + c * sz:][:sz].tobytes(), (c, k)
            assert sa[c] == sb[c], c


# ------------------------------------------------------------------ 5. role errors
def test_a_masked_frame_is_an_error_in_the_client_role_only(ctx, cuda):
    rng = random.Random(5)
    prefix = sframe(BIN, b"fine") + sframe(PING, b"p") + sframe(TEXT, b"open", fin=0)
    masked = frame(CONT, b"from a client", key=key(rng))
    wire = prefix + masked + sframe(BIN, b"never")
    conns = Conns(cuda, 2)
    outs, _, _ = run(ctx, cuda, conns, [dict(wire=wire, conn=0), dict(wire=prefix, conn=1)])
    r, d = outs[0]["res"], outs[0]["dres"]
    assert (r["status"], d["status"], d["err_off"], d["consumed"], r["resume_off"]) == \
        (MASKED, MASKED, len(prefix), len(prefix), len(prefix))
    assert d["n_frames"] == 3 and r["err_frame"] == NONE
    # the prefix is delivered exactly as without the error behind it
    assert outs[0]["units"] == outs[1]["units"] and plain(outs[0]["units"]) == [(BIN, b"fine"), (PING, b"p")]
    assert (outs[0]["dst"], outs[0]["ctl"], outs[0]["state"]) == (outs[1]["dst"], outs[1]["ctl"], outs[1]["state"])
    assert r["open_opcode"] == TEXT and r["open_len"] == 4
    # the same server frames through the server call: nothing moved
    servers = fm.Conns(cuda, 1)
    outs, _, _ = fm.run(ctx, cuda, servers, [dict(wire=prefix, conn=0)])
    assert outs[0]["res"]["status"] == outs[0]["dres"]["status"] == _lib.FWS_ERR_NOT_MASKED
    assert outs[0]["dres"]["err_off"] == 0 and outs[0]["res"]["n_msgs"] == 0


# ------------------------------------------------------------------ 6. frames the reference wrote
def test_the_reference_servers_frames_decode_to_the_recorded_payloads(ctx, cuda):
    with gzip.open(GOLDEN, "rt") as f:
        sess = [s for s in json.load(f) if s["server"]][0]
    tx, wire, want, cur = orc.OrcTx(is_server=True), bytearray(), [], None
    for r in sess["frames"]:
        p = np.random.default_rng(r["seed"]).integers(0, 256, r["len"], dtype=np.uint8).tobytes()
        b = tx.frame(p, r["frame_type"], r["last"], r["key"])
        # the bytes are the ones the compiled reference wrote
        assert len(b) == r["size"]
        if "hex" in r:
            assert b.hex() == r["hex"]
        else:
            assert b[:64].hex() == r["head_hex"] and hashlib.sha256(b).hexdigest() == r["sha256"]
        wire += b
        if r["frame_type"] >= 8:
            want.append((r["frame_type"], p))
            continue
        cur = (cur[0], cur[1] + p) if cur else (r["frame_type"], p)
        if r["last"]:
            want.append(cur)
            cur = None
    assert cur is None and want[-1][0] == CLOSE
    wire = bytes(wire)
    max_read = FULL - _lib.FWS_MSG_FLOW_MAX_PENDING - 16
    flow = gpu.MessageFlow(ctx, 1, max_read=max_read, role="client")
    got = []
    for at in range(0, len(wire), max_read):
        got += flow.feed({0: wire[at:at + max_read]})[0]
    assert [(op, body) for op, body, _ in got] == want
    assert flow.status == [0] and int(gpu.read_msg_flow(flow.flows, 0)["msg"]["wire_bytes"]) == len(wire)


# ------------------------------------------------------------------ 7. the two roles on the same payloads
def test_client_decode_of_c_equals_server_decode_of_c_with_a_zero_key(ctx, cuda):
    made = [cr.random_server_stream(seed, edges=(0, 125, 126)) for seed in range(8)]
    C_ = [w for w, _, _ in made] + [cr.twelve_frames()]
    S = [cr.to_server_role(w) for w in C_]
    n = len(C_)
    clients, servers = Conns(cuda, n), fm.Conns(cuda, n)
    caps = [dict(cap=len(w) // 2 + 16, msg_cap=len(w) // 2 + 16, dst_cap=len(w) + 16, ctl_cap=len(w) + 16) for w in C_]
    co, a, cs = run(ctx, cuda, clients, [dict(wire=w, conn=c, **caps[c]) for c, w in enumerate(C_)])
    so, b, ss = fm.run(ctx, cuda, servers, [dict(wire=w, conn=c, **caps[c]) for c, w in enumerate(S)])
    for c in range(n):
        for k in ("dst", "ctl", "msgs"):
            assert a.region(a.got, a.reads[c], k) == b.region(b.got, b.reads[c], k), (c, k)
        x, y = dict(co[c]["res"]), dict(so[c]["res"])
        assert x.pop("resume_off") == len(C_[c]) and y.pop("resume_off") == len(S[c]) and x == y
        fa = np.frombuffer(co[c]["frames"], dtype=_lib.FRAME_INFO)
        fb = np.frombuffer(so[c]["frames"], dtype=_lib.FRAME_INFO)
        assert len(fa) == len(fb) > 0
        for k in ("payload_len", "key", "opcode", "fin", "flags"):
            assert np.array_equal(fa[k], fb[k]), (c, k)
        assert np.array_equal(fa["hdr_len"] + 4, fb["hdr_len"])
        assert np.array_equal(fa["hdr_off"] + 4 * np.arange(len(fa), dtype=np.uint64), fb["hdr_off"])
        # the states: the same but for the wire bytes counted
        sa, sb = dict(co[c]["state"]["msg"]), dict(so[c]["state"]["msg"])
        assert sa.pop("wire_bytes") == len(C_[c]) and sb.pop("wire_bytes") == len(S[c]) and sa == sb


# ------------------------------------------------------------------ 8. masked replies
@pytest.mark.parametrize("strict", [False, True], ids=["multi", "strict"])
@pytest.mark.parametrize("flags", [0, CONTROL, ECHO, BOTH], ids=["none", "control", "echo", "both"])
def test_header_forms_and_control_payloads(ctx, cuda, flags, strict):
    rng = random.Random(81)
    sizes = (0, 1, 15, 16, 17, 125, 126, 65535, 65536)
    wires = [sframe(BIN, cc.payload(rng, n)) for n in sizes]
    wires += [sframe(PING, cc.payload(rng, n)) for n in (0, 1, 125)]
    wires += [sframe(PONG, b"pong")]
    closes = [b"", struct.pack(">H", 1000), struct.pack(">H", 4999) + cc.random_text(rng, 123)]
    wires += [sframe(CLOSE, p) for p in closes]
    n = len(wires)
    conns, rc = Conns(cuda, n), RConns(cuda, n, flags, strict)
    _, r = step(ctx, cuda, conns, rc, [dict(wire=w, conn=c) for c, w in enumerate(wires)], some_keys(rng, n))
    echo, ctl = int(bool(flags & ECHO)), int(bool(flags & CONTROL))
    assert [o["res"]["n_frames"] for o in r.outs] == [echo] * 9 + [ctl] * 3 + [0] + [ctl] * 3
    if flags & ECHO:
        assert [o["records"][0]["hdr_len"] for o in r.outs[:9]] == [6, 6, 6, 6, 6, 6, 8, 8, 14]
        assert [o["res"]["out_len"] for o in r.outs[:9]] == [h + s for h, s in zip([6] * 6 + [8, 8, 14], sizes)]
        assert [int(o["records"][0]["key"]) for o in r.outs[:3]] == [0, 0xFFFFFFFF, r.keys[2]]
    if ctl:
        assert [rf.state["close_code"] for rf in rc.ref[13:]] == [1005, 1000, 4999]
        assert walk_client_frames(r.region(10))[0][:3] == (PONG, 1, wires[10][2:])


LENGTHS = (0, 1, 3, 4, 15, 16, 17, 125, 126, 127, 4095, 4096, 65535, 65536)


@pytest.mark.parametrize("strict", [False, True], ids=["multi", "strict"])
@pytest.mark.parametrize("max_len", [SMALL, FULL], ids=["small", "full"])
def test_source_misalignment_and_payload_length_sweep(ctx, cuda, max_len, strict):
    """Read (mis, n): a message of mis bytes, then one of n bytes, whose echo's
    source is dst + mis, then one of 37: the frame of n bytes starts at region
    offset 6 + mis, its payload 6 | 8 | 14 bytes on, the next frame wherever that
    ends, so every source phase meets every seam phase and both header-length
    boundaries."""
    rng = random.Random(82)
    lengths = [n for n in LENGTHS if 16 + n + 37 + 3 * 10 <= max_len]
    assert len(lengths) == (12 if max_len == SMALL else 14)
    bodies = {n: cc.payload(rng, n) for n in lengths}
    reads, want = [], []
    for n in lengths:
        for mis in range(16):
            parts = [cc.payload(rng, mis), bodies[n], cc.payload(rng, 37)]
            reads.append(dict(wire=b"".join(sframe(BIN, p) for p in parts), conn=len(reads)))
            want.append(parts)
    conns, rc = Conns(cuda, len(reads)), RConns(cuda, len(reads), ECHO, strict)
    keys = some_keys(rng, len(reads))
    outs, r = step(ctx, cuda, conns, rc, reads, keys, max_len)
    assert all(o["entries"][1]["off"] & 15 == i % 16 for i, o in enumerate(outs))
    for i, parts in enumerate(want):
        got = walk_client_frames(r.region(i))
        assert [(op, fin, p) for op, fin, p, _ in got] == [(BIN, 1, p) for p in parts], i
        assert [k for *_, k in got] == [FRAG_KEY(keys[i], j) for j in range(3)], i


@FORMS
def test_258_masked_frames_and_the_key_of_each(ctx, cuda, max_len):
    rng = random.Random(83)
    opener = sframe(BIN, cc.payload(rng, 30))
    ones = [sframe(TEXT if j % 3 else BIN, bytes([65 + j % 26])) for j in range(256)]
    part = sframe(BIN, b"z", fin=0)
    conns, rc = Conns(cuda, 3), RConns(cuda, 3)
    step(ctx, cuda, conns, rc, [dict(wire=opener[:16], conn=c) for c in range(3)], [1, 2, 3], max_len)
    reads = [dict(wire=opener[16:] + b"".join(ones), conn=0),              # 257 entries
             dict(wire=opener[16:] + b"".join(ones[:255]) + part, conn=1),  # 256 and an open part
             dict(wire=opener[16:] + b"".join(ones), conn=2)]               # 257 and an open part, by hand
    by_hand = dict(open_opcode=BIN, open_len=1, open_off=0)
    keys = [0x9E3779B9, 0xFFFFFFFF, rng.getrandbits(32)]
    outs, r = step(ctx, cuda, conns, rc, reads, keys, max_len, opts=[{}, {}, dict(mres=by_hand)])
    assert [len(o["entries"]) for o in outs] == [257, 256, 257]
    assert [o["res"]["n_frames"] for o in r.outs] == [257, 257, 258]
    for i in range(3):
        got = walk_client_frames(r.region(i))
        assert [k for *_, k in got] == [FRAG_KEY(keys[i], j) for j in range(len(got))]
        assert [int(k) for k in r.outs[i]["records"]["key"]] == [k for *_, k in got]
    assert len({k for *_, k in walk_client_frames(r.region(2))}) == 258
    assert [x.tx["last_msg_not_fin"] for x in rc.ref] == [0, 1, 1]


@pytest.mark.parametrize("strict", [False, True], ids=["multi", "strict"])
def test_capacity_one_byte_short_writes_nothing(ctx, cuda, strict):
    rng = random.Random(84)
    wire = sframe(BIN, cc.payload(rng, 200)) + sframe(PING, b"ping") + sframe(TEXT, b"part", fin=0)
    need = (200 + 8) + (4 + 6) + (4 + 6)
    conns, rc = Conns(cuda, 2), RConns(cuda, 2, BOTH, strict)
    _, m, _ = run(ctx, cuda, conns, [dict(wire=wire, conn=0), dict(wire=wire, conn=1)])
    r = reply(ctx, cuda, m, rc, [7, 7], opts=[dict(out_cap=need - 1), dict(out_cap=need)])   # (check: the guards)
    assert r.outs[0]["res"] == tr.refusal(CAPACITY, 3, need) and r.outs[1]["res"]["out_len"] == need
    assert rc.ref[0].tx == rr.new_tx() and rc.ref[1].tx["wire_bytes"] == need and rc.ref[1].tx["last_msg_not_fin"] == 1
    assert rc.ref[0].state["close_sent"] == 0


@FORMS
def test_every_failure_code_is_an_eight_byte_masked_close(ctx, cuda, max_len):
    rng = random.Random(85)
    ok = sframe(BIN, b"answered")
    cases = [(ok + sframe(TEXT, b"\xc3("), 1007, 1),                          # a TEXT message that is not UTF-8
             (ok + sframe(TEXT, b"\xe2\x82", fin=0), 0, 2),                   # a cut sequence is no error yet
             (ok + sframe(TEXT, b"\xff!", fin=0), 1007, 1),                   # the open part, failed early
             (ok + sframe(BIN, cc.payload(rng, 301)), 1009, 1),               # a message over the limit
             (ok + sframe(BIN, b"", fin=0)[:1] + bytes([127]) + struct.pack(">Q", 1 << 20), 1009, 1),   # announced
             (ok + sframe(CLOSE, b"\x03"), 1002, 1),                          # a CLOSE of one byte
             (ok + sframe(CLOSE, struct.pack(">H", 1005)), 1002, 1),          # a code that may not appear
             (ok + sframe(CLOSE, struct.pack(">H", 1000) + b"\xff"), 1007, 1),   # a reason that is not UTF-8
             (ok + sframe(BIN, b"x", rsv=4), 1002, 1),                        # RSV
             (ok + frame(BIN, b"masked", key=key(rng)), 1002, 1),             # FWS_ERR_MASKED: this role's error
             (ok + sframe(CONT, b"x"), 1002, 1),                              # a continuation of nothing
             (ok + sframe(PING, b"x", fin=0), 1002, 1),                       # a fragmented control frame
             (ok + bytes([0x83, 0]), 1002, 1),                                # an opcode that does not exist
             (ok + bytes([0x82, 127]) + struct.pack(">Q", (1 << 32) + 1), 1009, 1)]   # FWS_ERR_TOO_LARGE
    n = len(cases)
    conns, rc = Conns(cuda, n), RConns(cuda, n, BOTH, strict=True, limit=300)
    keys = some_keys(rng, n)
    outs, r = step(ctx, cuda, conns, rc, [dict(wire=w, conn=c) for c, (w, _, _) in enumerate(cases)], keys, max_len)
    assert outs[9]["res"]["status"] == MASKED and outs[13]["res"]["status"] == _lib.FWS_ERR_TOO_LARGE
    for c, (_, code, at) in enumerate(cases):
        got = walk_client_frames(r.region(c))
        assert rc.ref[c].state["fail_code"] == code and got[0][:3] == (BIN, 1, b"answered"), c
        if not code:
            assert rc.ref[c].state["close_sent"] == 0
            continue
        k = FRAG_KEY(keys[c], at).to_bytes(4, "little")
        tail = bytes([0x88, 0x82]) + k + bytes(x ^ y for x, y in zip(struct.pack(">H", code), k))
        assert len(got) == at + 1 and r.region(c)[-8:] == tail and got[-1][:3] == (CLOSE, 1, struct.pack(">H", code)), c
        assert rc.ref[c].state["close_sent"] == 1


# ------------------------------------------------------------------ 9. two responders talk to each other
def test_a_client_and_a_server_responder_on_one_device(ctx, cuda):
    rng = random.Random(9)
    n, max_read = 4, 4096
    sender = gpu.MessageSender(ctx, n, max_send=32 << 10)
    server = gpu.MessageResponder(gpu.MessageFlow(ctx, n, max_read=max_read), BOTH)
    picked = {}

    def key_fn(conn):
        picked[conn] = rng.getrandbits(32)
        return picked[conn]

    client_flow = gpu.MessageFlow(ctx, n, max_read=max_read, role="client")
    client = gpu.MessageResponder(client_flow, CONTROL, key_fn=key_fn)
    assert client_flow.cap == 256 and client.out_slot > server.out_slot
    with pytest.raises(ValueError):
        gpu.MessageResponder(server.flow, BOTH, key_fn=key_fn)
    with pytest.raises(ValueError):
        gpu.MessageFlow(ctx, n, max_read=max_read, role="proxy")
    sent = [[(BIN, cc.payload(rng, 700)), (PING, b"alive?"), (TEXT, cc.random_text(rng, 333))],
            [(TEXT, cc.random_text(rng, 10000)), (BIN, b"")],
            [(PING, b""), (BIN, cc.payload(rng, 4096)), (CLOSE, struct.pack(">H", 1000) + b"done"), (BIN, b"late")],
            [(BIN, cc.payload(rng, 1)), (PONG, b"unasked"), (PING, cc.payload(rng, 125))]]
    to_server = [b"" for _ in range(n)]
    for k in range(max(map(len, sent))):
        out = sender.send({c: (s[k][0], s[k][1], True) for c, s in enumerate(sent) if k < len(s)}, max_frame=3000,
                          masked=True)
        for c, b in out.items():
            to_server[c] += b

    def pump(responder, wires, units, replies):
        """The wires through the responder in random reads."""
        pos = [0] * n
        while any(p < len(w) for p, w in zip(pos, wires)):
            reads = {}
            for c, w in enumerate(wires):
                if pos[c] < len(w):
                    k = rng.randint(1, max_read)
                    reads[c] = w[pos[c]:pos[c] + k]
                    pos[c] += k
            got, back = responder.feed(reads)
            for c in reads:
                units[c] += got[c]
                if responder is client:               # the bytes are predictable: frame j under FRAG_KEY(key, j)
                    assert [f[3] for f in walk_client_frames(back[c])] == \
                        [FRAG_KEY(responder.last_keys[c], j) for j in range(len(walk_client_frames(back[c])))]
                    assert responder.last_keys[c] == picked[c]
                replies[c] += back[c]

    # client -> server: the server echoes and answers
    s_units, to_client = [[] for _ in range(n)], [b""] * n
    pump(server, to_server, s_units, to_client)
    answered = []
    for c, s in enumerate(sent):
        assert [(op, body) for op, body, _ in s_units[c]] == s, c
        want = []
        for op, body in s:
            if op != PONG:
                want.append((PONG if op == PING else op, body))
            if op == CLOSE:
                break
        assert messages(walk_frames(to_client[c])) == (want, None), c
        answered.append(want)
    # server -> client, cut at random bytes: the client's units, its masked PONGs and CLOSE
    c_units, back_to_server = [[] for _ in range(n)], [b""] * n
    pump(client, to_client, c_units, back_to_server)
    for c in range(n):
        assert [(op, body) for op, body, _ in c_units[c]] == answered[c] and client_flow.status[c] == 0, c
        got = [(op, fin, p) for op, fin, p, _ in walk_client_frames(back_to_server[c])]
        assert got == [(op, 1, p) for op, p in answered[c] if op == CLOSE], c    # (the server sent no PING)
    # ... and a PING from the server's application, answered by the client with a masked PONG
    ping = sframe(PING, b"are you there")
    got, back = client.feed({0: ping, 1: ping, 3: ping})
    for c in (0, 1, 3):
        assert got[c] == [(PING, b"are you there", False)]
        assert [f[:3] for f in walk_client_frames(back[c])] == [(PONG, 1, b"are you there")]
        back_to_server[c] += back[c]
    # client -> server again: decoded with status 0 to the expected units
    final, nothing = [[] for _ in range(n)], [b""] * n
    pump(server, back_to_server, final, nothing)
    for c in range(n):
        want = [(CLOSE, p, False) for op, p in answered[c] if op == CLOSE]
        if c != 2:
            want.append((PONG, b"are you there", False))
        assert final[c] == want and server.flow.status[c] == 0, c
    assert nothing == [b""] * n                       # the server's CLOSE was sent already; a PONG is not answered
    for r in (server, client):
        st = [gpu.read_reply_state(r.states, c) for c in range(n)]
        assert [int(s["close_sent"]) for s in st] == [0, 0, 1, 0] and int(st[2]["close_code"]) == 1000


# ------------------------------------------------------------------ 10. capture
def test_graph_capture_of_client_decode_and_reply(cuda):
    """client decode + client reply captured once, replayed on two inputs that
    differ in every payload byte, in the keys and in the states; no reset node."""
    n = 6

    def inputs(seed):
        rng = random.Random(seed)
        return [dict(wire=sframe(BIN, cc.payload(rng, 10 + 30 * c)) + sframe(PING, cc.payload(rng, c)) +
                     sframe(TEXT, cc.random_text(rng, 50), fin=0), conn=c) for c in range(n)]

    c = gpu.Ctx(0)
    try:
        eager = []
        for seed in (21, 22):
            conns, rc = Conns(cuda, n), RConns(cuda, n)
            if seed == 22:                            # the second input finds messages open
                run(c, cuda, conns, [dict(wire=sframe(BIN, b"first", fin=0), conn=k) for k in range(n)])
                for k in range(n):
                    rc.ref[k].tx["last_msg_not_fin"] = 1
                rc.tx[0:rc.n_dev * rp.TSZ:2 * rp.TSZ] = 1
                rc.check()
                reads = [dict(r, wire=sframe(CONT, b"", fin=1) + r["wire"]) for r in inputs(seed)]
            else:
                reads = [dict(r, wire=sframe(PONG, b"") + r["wire"]) for r in inputs(seed)]
            before = (conns.t.clone(), rc.tx.clone(), rc.st.clone())
            m = Flow(cuda, conns, reads)
            m.expect()
            r = Reply(cuda, m, rc, [random.Random(seed).getrandbits(32) + k for k in range(n)])
            r.expect()
            clean = (m.arena.clone(), r.arena.clone(), r.kt.clone())
            m.launch(c)
            r.launch(c)
            torch.cuda.synchronize()
            m.check()
            r.check()
            rc.check()
            eager.append(dict(m=m, r=r, conns=conns, rc=rc, before=before, clean=clean,
                              after=(m.arena.clone(), r.arena.clone(), conns.t.clone(), rc.tx.clone(), rc.st.clone())))
        a, b = eager
        assert a["m"].sec == b["m"].sec and a["r"].sec == b["r"].sec            # one layout: one graph serves both
        assert [x["at"] for x in a["m"].reads] == [x["at"] for x in b["m"].reads]
        m, r, conns, rc = a["m"], a["r"], a["conns"], a["rc"]
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            m.launch(c)
            r.launch(c)
        torch.cuda.synchronize()
        for e in (a, b, a):
            for t, src in zip((m.arena, r.arena, r.kt, conns.t, rc.tx, rc.st), e["clean"] + e["before"]):
                t.copy_(src)
            g.replay()
            torch.cuda.synchronize()
            for t, want in zip((m.arena, r.arena, conns.t, rc.tx, rc.st), e["after"]):
                assert torch.equal(t, want)
        assert not torch.equal(a["after"][1], b["after"][1])
    finally:
        torch.cuda.synchronize()
        c.close()
