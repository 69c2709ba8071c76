"""GPU parity of fws_gpu_decode_messages_flow: the one-launch, many-connections
message decode that resumes inside a frame.

The oracle is FlowRef (msgflow_ref.py), one per connection; test_msg_flow_cpu.py
holds it against the reference's OnRecvData. Every call lays its buffers out as
the multi tests do (Multi of test_gpu_msg_multi.py: one arena, every buffer
followed by guard bytes) and checks, per read: the wire unchanged, every guard,
every fws_msg_result / fws_decode_result / fws_msg_info field, the frame
records, dst and ctl; the states lie in an array whose odd records are guards
and are compared byte for byte (all 96). All comparisons are exact."""
import random
import struct

import numpy as np
import pytest
import torch

import test_gpu_msg_carry as cc
import test_gpu_msg_multi as mm
from flashws_amd import _lib, gpu
from msgflow_ref import FlowRef, state_bytes
from test_gpu_msg_carry import (BIN, CLOSE, CONT, FILL, GUARD, NONE, PING, PONG, TEXT, frame, random_cuts,
                                random_stream, twelve_frames, whole)
from test_gpu_msg_multi import DSZ, ESZ, RSZ, fill, key

pytestmark = pytest.mark.gpu

CAPACITY, DECLINED, INVALID, SEQUENCE = (_lib.FWS_ERR_CAPACITY, _lib.FWS_ERR_DECLINED, _lib.FWS_ERR_INVALID,
                                         _lib.FWS_ERR_SEQUENCE)
SMALL, FULL = mm.SMALL, mm.FULL
SSZ = _lib.MSG_FLOW.itemsize
FORMS = pytest.mark.parametrize("max_len", [SMALL, FULL], ids=["small", "full"])
KEY4 = 0xD4C3B2A1                                         # four distinct key bytes


class Conns:
    """The connections of a test: their states on the device -- record 2c is
    connection c's, the odd records are guards -- and their references."""

    def __init__(self, cuda, n):
        self.n, self.n_dev = n, 2 * n
        host = np.full(self.n_dev * SSZ + GUARD, FILL, dtype=np.uint8)
        for c in range(n):
            host[2 * c * SSZ:(2 * c + 1) * SSZ] = 0
        self.t = torch.from_numpy(host).to(cuda)
        self.ref = [FlowRef() for _ in range(n)]
        self.units = [[] for _ in range(n)]

    def check(self):
        raw = self.t.cpu().numpy().tobytes()
        out = []
        for c in range(self.n):
            rec, want = raw[2 * c * SSZ:(2 * c + 1) * SSZ], state_bytes(self.ref[c].state)
            if rec != want:
                got = np.frombuffer(rec, dtype=_lib.MSG_FLOW)[0]
                st = self.ref[c].state
                for k in _lib.MSG_CARRY.names:
                    assert int(got["msg"][k]) == st["msg"][k], (c, k, int(got["msg"][k]), st["msg"][k])
                for k in ("frame_unread", "frame_len", "frame_key", "frame_fin"):
                    assert int(got[k]) == st[k], (c, k, int(got[k]), st[k])
                assert rec == want, ("pad / reserved", c)
            assert raw[(2 * c + 1) * SSZ:(2 * c + 2) * SSZ] == fill * SSZ, ("the guard behind state", c)
            out.append(rec)
        assert raw[self.n_dev * SSZ:] == fill * GUARD
        return out


class Flow(mm.Multi):
    """One call in Multi's arena, launched as the flow call and checked against FlowRef."""

    def launch(self, ctx, stream=None):
        rc = gpu.decode_messages_flow(ctx, self.arena, self.t("reads"), self.n, self.max_len, self.t("frames"),
                                      self.t("msgs"), self.arena, self.arena, self.t("res"), self.t("mres"),
                                      self.conns.t, self.conns.n_dev, stream=stream)
        assert rc == 0, rc

    def check(self):
        got = self.got = self.arena.cpu().numpy()
        for k in ("res", "mres", "reads"):
            o, sz = self.sec[k]
            assert got[o + sz:o + sz + GUARD].tobytes() == fill * GUARD, k
        o, sz = self.sec["reads"]
        assert got[o:o + sz].tobytes() == self.host_in.numpy()[o:o + sz].tobytes(), "the descriptors were modified"
        res = np.frombuffer(got[self.sec["res"][0]:][:self.n * DSZ].tobytes(), dtype=_lib.DECODE_RESULT)
        mres = np.frombuffer(got[self.sec["mres"][0]:][:self.n * RSZ].tobytes(), dtype=_lib.MSG_RESULT)
        for i, (r, out) in enumerate(zip(self.reads, self.outs)):
            n = len(r["wire"])
            assert self.region(got, r, "wire") == r["wire"] + fill * (max(n, 16) - n + GUARD), ("wire", i)
            if out is None:                           # declined / a bad descriptor: the two results, nothing else
                want = dict.fromkeys(_lib.MSG_RESULT.names, 0)
                want.update(status=r["expect"], err_frame=NONE, open_first_frame=NONE)
                for k in _lib.MSG_RESULT.names:
                    assert int(mres[i][k]) == want[k], (i, k, int(mres[i][k]))
                for k in _lib.DECODE_RESULT.names:
                    assert int(res[i][k]) == (r["expect"] if k == "status" else 0), (i, k, int(res[i][k]))
                for k in ("dst", "ctl", "frames", "msgs"):
                    reg = self.region(got, r, k)
                    assert reg == fill * len(reg), (k, i)
                continue
            for k in _lib.MSG_RESULT.names:
                assert int(mres[i][k]) == out["res"][k], (i, k, int(mres[i][k]), out["res"][k])
            for k in _lib.DECODE_RESULT.names:
                assert int(res[i][k]) == out["dres"][k], (i, k, int(res[i][k]), out["dres"][k])
            assert self.region(got, r, "dst") == out["dst"] + fill * (r["dst_cap"] + GUARD - len(out["dst"])), ("dst", i)
            assert self.region(got, r, "ctl") == out["ctl"] + fill * (r["ctl_cap"] + GUARD - len(out["ctl"])), ("ctl", i)
            ne = min(len(out["entries"]), r["msg_cap"])
            reg = self.region(got, r, "msgs")
            em = np.frombuffer(reg[:ne * ESZ], dtype=_lib.MSG_INFO)
            for j in range(ne):
                for k in _lib.MSG_INFO.names:
                    assert int(em[j][k]) == out["entries"][j][k], (i, j, k, int(em[j][k]), out["entries"][j][k])
            assert reg[ne * ESZ:] == fill * (len(reg) - ne * ESZ), ("entries past the count", i)
            reg, recs = self.region(got, r, "frames"), out["frames"]
            assert reg[:len(recs)] == recs, ("frame records", i)
            assert reg[len(recs):] == fill * (len(reg) - len(recs)), ("frames past the count", i)
        return mres


def run(ctx, cuda, conns, reads, max_len=None):
    """One call, checked in full: returns (the references' outputs, the call, the states' bytes)."""
    m = Flow(cuda, conns, reads, max_len)
    outs = m.expect()
    m.launch(ctx)
    m.check()
    return outs, m, conns.check()


def feed_all(ctx, cuda, conns, streams, cuts, max_len=None, **caps):
    """Connection c gets streams[c] cut at cuts[c]: call k serves every
    connection's pending bytes and its bytes up to its k-th cut, in one launch.
    Returns the outputs per call."""
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
    return [(op, body, ok) for op, body, ok, _ in units]


# ------------------------------------------------------------------ 1. whole frames: the multi call
def whole_frame_reads(seed):
    """Two reads of whole frames: the first ends after the first fragment of a
    fragmented message (the second starts with a carried message), the second
    ends, by seed, with nothing, a partial header or a cut control frame."""
    wire, spans, fragmented = random_stream(seed)
    rng = random.Random(500 + seed)
    at = spans[fragmented[0][0]][1]
    tail = [b"", frame(BIN, b"x" * 200, key=key(rng))[:rng.randint(1, 7)],
            frame(PING, cc.payload(rng, 40), key=key(rng))[:rng.randint(6, 45)],
            frame(CLOSE, struct.pack(">H", 1001), key=key(rng))[:rng.randint(1, 5)]][seed % 4]
    return wire[:at], wire[at:] + tail


@FORMS
@pytest.mark.parametrize("seed", range(40))
def test_equals_the_multi_call_on_whole_frames(ctx, cuda, seed, max_len):
    a, b = whole_frame_reads(seed)
    flows, carries = Conns(cuda, 1), mm.Conns(cuda, 1)
    for wire in (a, b):
        _, f, states = run(ctx, cuda, flows, [dict(wire=wire, conn=0)], max_len)
        _, m, cs = mm.run(ctx, cuda, carries, [dict(wire=wire, conn=0)], max_len)
        assert f.sec == m.sec and f.reads[0]["at"] == m.reads[0]["at"]
        # the two arenas: the same layout, the same inputs, every byte written the same
        assert f.got.tobytes() == m.got.tobytes()
        assert states[0][:mm.CSZ] == cs[0] and states[0][mm.CSZ:] == bytes(SSZ - mm.CSZ)
    assert flows.units[0][:len(carries.units[0])] == carries.units[0] and flows.ref[0].state["msg"]["open_opcode"] == 0


# ------------------------------------------------------------------ 2. every cut at once
@FORMS
def test_every_cut_at_once(ctx, cuda, max_len):
    stream = twelve_frames()
    L = len(stream)
    units, status, _ = whole(stream)
    assert status == 0
    conns = Conns(cuda, L + 1)
    calls = feed_all(ctx, cuda, conns, [stream] * (L + 1), [[c] for c in range(L + 1)], max_len)
    in_frame = sum(1 for o in calls[0] if o["state"]["frame_unread"])
    leads = sum(1 for o in calls[1] for e in o["entries"] if e["flags"] and e["first_frame"] == NONE)
    assert in_frame > 40 and leads > 10
    for c in range(L + 1):
        assert conns.units[c] == units, c
        st = conns.ref[c].state
        assert st["msg"]["wire_bytes"] == L and st["frame_unread"] == 0 and calls[-1][c]["res"]["status"] == 0


def test_cut_in_three_over_a_stride(ctx, cuda):
    stream = twelve_frames()
    units = whole(stream)[0]
    cuts = [[a, b] for a in range(1, len(stream), 13) for b in range(a + 1, len(stream), 17)]
    conns = Conns(cuda, len(cuts))
    feed_all(ctx, cuda, conns, [stream] * len(cuts), cuts)
    for c in range(len(cuts)):
        assert conns.units[c] == units and conns.ref[c].state["msg"]["wire_bytes"] == len(stream), cuts[c]


# ------------------------------------------------------------------ 3. key phase and seams
@FORMS
def test_key_phase_and_seams(ctx, cuda, max_len):
    rng = random.Random(3)
    streams, cuts, want = [], [], []
    for present in (0, 1, 2, 3, 4, 15, 16, 17, 33):
        for rest in (1, 2, 3, 5, 13, 16, 18):         # the lead's length: up to one dst chunk and beyond
            for op in (TEXT, BIN):
                n = present + rest + 21
                body = cc.random_text(rng, n) if op == TEXT else cc.payload(rng, n)
                first = frame(op, body[:present + rest], fin=0, key=KEY4)
                s = first + frame(CONT, body[present + rest:present + rest + 1], fin=0, key=key(rng))
                s += frame(CONT, b"", fin=0, key=key(rng))
                s += frame(CONT, body[present + rest + 1:], fin=1, key=key(rng))
                cut = len(first) - rest
                streams.append(s)
                # in two: the cut frame, then the lead and the three frames in one read; in three: the lead
                # ends exactly at the end of its read
                cuts.append([cut] if len(streams) % 2 else [cut, len(first)])
                want.append([(op, body, int(op == TEXT), 4)])
    conns = Conns(cuda, len(streams))
    calls = feed_all(ctx, cuda, conns, streams, cuts, max_len)
    for c, s in enumerate(streams):
        assert conns.units[c] == want[c] == whole(s)[0], c
    first = calls[0]
    assert len({o["state"]["frame_key"] for o in first}) == 4 and len(set(KEY4.to_bytes(4, "little"))) == 4   # every phase
    assert any(o["res"]["open_len"] == 0 and o["state"]["frame_unread"] for o in first)   # payload starts at len
    assert any(o["dres"]["n_frames"] == 0 and o["state"]["frame_unread"] == 0 for o in calls[1])  # lead ends at len


# ------------------------------------------------------------------ 4. a frame larger than the stage
BIG_FRAMES = {}


def big_frames():
    """(wire, body, verdict) of a 300 KiB TEXT frame, a 70 000-byte one and a
    70 000-byte one with an ill-formed sequence; made once."""
    if not BIG_FRAMES:
        rng = random.Random(4)
        a, b = cc.random_text(rng, 300 << 10), cc.random_text(rng, 70000)
        bad = bytearray(b)
        at = next(i for i in range(40000, 70000) if bad[i] >= 0xE0)
        bad[at + 1] = 0x28                            # a lead byte followed by '('
        BIG_FRAMES["v"] = [(frame(TEXT, x, key=key(rng)), bytes(x), cc.strict_ok(x)) for x in (a, b, bytes(bad))]
        assert [v[2] for v in BIG_FRAMES["v"]] == [1, 1, 0] and len(BIG_FRAMES["v"][0][0]) == (300 << 10) + 14
    return BIG_FRAMES["v"]


def test_a_frame_larger_than_the_stage(ctx, cuda):
    cases = big_frames()
    rng = random.Random(44)
    hi = FULL - _lib.FWS_MSG_FLOW_MAX_PENDING
    cuts = []
    for j, (w, _, _) in enumerate(cases):
        at, cs = 0, []
        sizes = [5, hi, 1, 17] + [rng.randint(1, hi) for _ in range(8)] if j == 0 else \
            [9, 3, 1] + [rng.randint(1, 20000) for _ in range(12)]
        for size in sizes:
            at += size
            if at < len(w):
                cs.append(at)
        cuts.append(cs)
    conns = Conns(cuda, len(cases))
    calls = feed_all(ctx, cuda, conns, [w for w, _, _ in cases], cuts, FULL)
    payload_only = sum(1 for outs in calls for o in outs if o["dres"]["n_frames"] == 0 and o["res"]["data_bytes"])
    assert payload_only >= 4
    for c, (w, body, ok) in enumerate(cases):
        assert conns.units[c] == [(TEXT, body, ok, 1)], c
        assert conns.ref[c].state["msg"]["wire_bytes"] == len(w) and conns.ref[c].state["frame_unread"] == 0
    hdr_len = _lib.FRAME_INFO.fields["hdr_len"][1]
    assert calls[1][0]["state"]["frame_len"] == 300 << 10 and calls[1][0]["frames"][hdr_len] == 14   # the 64-bit form


# ------------------------------------------------------------------ 5. UTF-8 at an in-frame cut
@FORMS
def test_utf8_sequence_split_inside_a_frame(ctx, cuda, max_len):
    rng = random.Random(5)
    streams, cuts, want = [], [], []
    for seq in cc.VALID + cc.ILL_FORMED:
        for pre, post in ((b"", b""), (b"ab", b"cd"), (b"", b"cd"), (b"ab", b"")):
            body = pre + seq + post
            s = frame(TEXT, body, key=key(rng))
            for at in range(len(seq) + 1):            # the cut before byte `at` of the sequence
                streams.append(s)
                cuts.append([6 + len(pre) + at])
                want.append([(TEXT, body, int(seq in cc.VALID), 1)])
    conns = Conns(cuda, len(streams))
    calls = feed_all(ctx, cuda, conns, streams, cuts, max_len)
    assert sum(1 for o in calls[0] if o["state"]["frame_unread"]) >= len(streams) - 2 * len(cc.VALID + cc.ILL_FORMED)
    assert any(o["state"]["msg"]["utf8_bad"] for o in calls[0])
    for c in range(len(streams)):
        assert conns.units[c] == want[c], (c, streams[c], cuts[c])


# ------------------------------------------------------------------ 6. control frames wait whole
def test_control_frames_wait_whole(ctx, cuda):
    rng = random.Random(6)
    msg = frame(BIN, b"before", key=key(rng))
    ping = frame(PING, b"are you there", key=key(rng))
    close = frame(CLOSE, struct.pack(">H", 1000), key=key(rng))
    text = cc.random_text(rng, 40)
    opener = frame(TEXT, text[:30], fin=0, key=key(rng))
    streams = [msg + ping + msg, msg + close, opener + ping + frame(CONT, text[30:], fin=1, key=key(rng))]
    cuts = [[len(msg) + 6 + 4], [len(msg) + 3], [len(opener) - 11]]
    conns = Conns(cuda, 3)
    calls = feed_all(ctx, cuda, conns, streams, cuts)
    for c in (0, 1):                                  # resume_off is the header, nothing of the frame is listed
        r = calls[0][c]["res"]
        assert (r["resume_off"], r["n_msgs"], r["ctl_bytes"], r["status"]) == (len(msg), 1, 0, 0)
        assert calls[0][c]["state"]["frame_unread"] == 0
    assert calls[0][0]["dres"]["carry_unread"] == 9 and calls[0][1]["dres"]["carry_hdr_len"] == 3
    assert plain(conns.units[0]) == [(BIN, b"before", 0), (PING, b"are you there", 0), (BIN, b"before", 0)]
    assert plain(conns.units[1]) == [(BIN, b"before", 0), (CLOSE, struct.pack(">H", 1000), 0)]
    # a PING behind a lead: delivered before the message it interrupts
    assert calls[0][2]["state"]["frame_unread"] == 11
    assert plain(conns.units[2]) == [(PING, b"are you there", 0), (TEXT, text, 1)]
    e = calls[1][2]["entries"]
    assert (e[0]["opcode"], e[0]["first_frame"]) == (PING, 0) and (e[1]["first_frame"], e[1]["last_frame"]) == (1, 1)


# ------------------------------------------------------------------ 7. errors
def test_errors_behind_a_lead_and_on_cut_frames(ctx, cuda):
    rng = random.Random(7)
    body = cc.payload(rng, 50)
    opener = frame(BIN, body, fin=0, key=KEY4)
    ok_msg = frame(BIN, b"fine", key=key(rng))
    cut = len(opener) - 20
    lead = opener[cut:]
    seconds = [
        (lead + frame(TEXT, b"new", key=key(rng)) + ok_msg, SEQUENCE, 0),                 # a start, a message open
        (lead + frame(TEXT, cc.random_text(rng, 30), key=key(rng))[:20], SEQUENCE, 0),    # the same, cut
        (lead + frame(CONT, b"x", fin=0, key=key(rng), rsv=4) + ok_msg, _lib.FWS_ERR_RSV, NONE),
        (lead + frame(PING, b"x", fin=0, key=key(rng)), _lib.FWS_ERR_CONTROL_FRAME, 0),
    ]
    conns = Conns(cuda, len(seconds) + 1)
    firsts = [dict(wire=opener[:cut], conn=c) for c in range(len(seconds))]
    # connection 4: nothing open, a cut continuation
    firsts.append(dict(wire=ok_msg + frame(CONT, cc.payload(rng, 30), key=key(rng))[:20], conn=len(seconds)))
    outs, _, _ = run(ctx, cuda, conns, firsts)
    r = outs[-1]["res"]
    assert (r["status"], r["err_frame"], r["resume_off"], r["n_data_frames"]) == (SEQUENCE, 1, len(ok_msg), 1)
    assert outs[-1]["state"]["frame_unread"] == 0 and outs[-1]["dst"] == b"fine"
    outs, _, _ = run(ctx, cuda, conns, [dict(wire=s[0], conn=c) for c, s in enumerate(seconds)])
    for c, (_, status, err_frame) in enumerate(seconds):
        r, st = outs[c]["res"], outs[c]["state"]
        assert (r["status"], r["err_frame"], r["resume_off"]) == (status, err_frame, 20), c
        # the state just before the failing header: the lead delivered, no frame in progress
        assert st["frame_unread"] == st["frame_len"] == st["frame_key"] == st["frame_fin"] == 0
        assert (st["msg"]["open_opcode"], st["msg"]["open_bytes"], st["msg"]["open_frames"]) == (BIN, 50, 1)
        assert outs[c]["dst"] == body[30:] and r["open_len"] == 20


def test_an_error_stays_on_its_connection(ctx, cuda):
    streams = [random_cuts(s) for s in range(16)]     # (wire, cuts): the first read ends at the first cut
    bad_opcode = bytes([0x83, 0x80, 1, 2, 3, 4])

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
    assert any(o["state"]["frame_unread"] for o in clean[0][0])
    for (_, a, sa), (_, b, sb) in zip(clean, dirty):
        for c in range(16):
            if c == 7:
                continue
            for k in ("dst", "ctl", "frames", "msgs"):
                assert a.region(a.got, a.reads[c], k) == b.region(b.got, b.reads[c], k), (c, k)
            for k, sz in (("res", DSZ), ("mres", RSZ)):
                o = a.sec[k][0] + c * sz
                assert a.got[o:o + sz].tobytes() == b.got[b.sec[k][0] + c * sz:][:sz].tobytes(), (c, k)
            assert sa[c] == sb[c], c


# ------------------------------------------------------------------ 8. capacities
def test_capacities_with_a_frame_in_progress(ctx, cuda):
    rng = random.Random(8)
    text = cc.random_text(rng, 60)
    opener = frame(TEXT, text, fin=1, key=KEY4)
    cut = len(opener) - 25
    tail = opener[cut:] + frame(PING, b"ping!", key=key(rng)) + frame(BIN, b"more", key=key(rng))
    conns = Conns(cuda, 5)
    run(ctx, cuda, conns, [dict(wire=opener[:cut], conn=c) for c in range(5)])
    assert all(r.state["frame_unread"] == 25 for r in conns.ref)
    short = {1: dict(dst_cap=28), 2: dict(ctl_cap=4), 3: dict(msg_cap=2), 4: dict(dst_cap=16)}
    before = conns.check()
    outs, _, after = run(ctx, cuda, conns, [dict(wire=tail, conn=c, **short.get(c, {})) for c in range(5)])
    for c in (1, 2, 3, 4):
        r = outs[c]["res"]
        assert (r["status"], r["resume_off"], r["n_msgs"], r["data_bytes"], r["ctl_bytes"]) == (CAPACITY, 0, 3, 29, 5)
        assert after[c] == before[c] and (outs[c]["dst"], outs[c]["ctl"]) == (b"", b"")   # (Flow.check: only fill)
    assert outs[0]["res"]["status"] == 0
    # the same bytes again with exact capacities
    outs, _, _ = run(ctx, cuda, conns, [dict(wire=b"" if c == 0 else tail, conn=c, dst_cap=32, ctl_cap=5, msg_cap=3)
                                        for c in range(5)])
    for c in range(5):
        assert plain(conns.units[c]) == [(TEXT, text, 1), (PING, b"ping!", 0), (BIN, b"more", 0)], c


def test_frame_capacity_is_continued_from_resume_off(ctx, cuda):
    rng = random.Random(81)
    head, tail = cc.capacity_stream(rng)
    stream = head + tail
    units = whole(stream)[0]
    conns = Conns(cuda, 1)
    pos, calls = 0, 0
    first = 40                                        # a cut inside a frame, then three frames to a call
    while pos < len(stream):
        end = first if calls == 0 else len(stream)
        outs, _, _ = run(ctx, cuda, conns, [dict(wire=stream[pos:end], conn=0, cap=3)])
        r = outs[0]["res"]
        assert r["resume_off"] > 0 and r["status"] in (0, CAPACITY)
        pos, calls = pos + r["resume_off"], calls + 1
    assert calls >= 5 and conns.units[0] == units and r["status"] == 0


@FORMS
def test_300_six_byte_frames_in_two_calls(ctx, cuda, max_len):
    rng = random.Random(82)
    ops = [(BIN, 0), (CONT, 0), (PING, 1), (CONT, 1), (TEXT, 1), (PONG, 1)]
    stream = b"".join(frame(op, b"", fin=fin, key=key(rng)) for op, fin in (ops[j % 6] for j in range(300)))
    assert len(stream) == 1800
    units, status, _ = whole(stream)
    assert status == 0 and len(units) == 200
    conns = Conns(cuda, 1)
    outs, _, _ = run(ctx, cuda, conns, [dict(wire=stream, conn=0)], max_len)
    r, d = outs[0]["res"], outs[0]["dres"]
    assert (r["status"], r["resume_off"], d["status"], d["n_frames"], d["consumed"]) == (CAPACITY, 1536, CAPACITY, 257, 1536)
    outs, _, _ = run(ctx, cuda, conns, [dict(wire=stream[1536:], conn=0)], max_len)
    assert outs[0]["res"]["status"] == 0 and outs[0]["dres"]["n_frames"] == 44
    assert conns.units[0] == units and conns.ref[0].state["msg"]["wire_bytes"] == 1800


# ------------------------------------------------------------------ 9. descriptors
def test_refused_descriptors_write_the_two_results_only(ctx, cuda):
    rng = random.Random(9)
    opener = frame(BIN, cc.payload(rng, 40), fin=0, key=key(rng))
    conns = Conns(cuda, 5)
    run(ctx, cuda, conns, [dict(wire=opener[:20], conn=c) for c in range(5)])     # a frame in progress everywhere
    rest = opener[20:]
    before = conns.check()
    reads = [dict(wire=rest, conn=0),
             dict(wire=b"\0" * 4 + rest, conn=1, expect=INVALID, misalign=4),
             dict(wire=rest, conn=2, expect=INVALID, desc=dict(conn=conns.n_dev)),
             dict(wire=rest, conn=3, expect=INVALID, desc=dict(dst_off=8)),
             dict(wire=rest + bytes(40), conn=4, expect=DECLINED)]
    outs, _, after = run(ctx, cuda, conns, reads, max_len=len(rest))
    assert outs[0]["res"]["status"] == 0 and outs[0]["state"]["frame_unread"] == 0
    assert after[1:] == before[1:] and after[0] != before[0]
    m = Flow(cuda, conns, [dict(wire=bytes(SMALL + 16), conn=1, expect=DECLINED)], SMALL)    # the small form's stage
    m.expect()
    m.launch(ctx)
    m.check()
    assert conns.check()[1] == before[1]


# ------------------------------------------------------------------ 10. ordering
def two_queued_calls(cuda, conns, n):
    firsts, seconds = [], []
    for c in range(n):
        rng = random.Random(1000 + c)
        text = cc.random_text(rng, 90 + 7 * c)
        s = cc.good_messages(rng, 1 + c % 4) + frame(TEXT, text, key=key(rng))
        cut = len(s) - 20 - c % 5 if c % 3 else len(s) + 7       # inside the TEXT frame; inside the PING behind it
        s += frame(PING, b"mid", key=key(rng)) + cc.good_messages(rng, 2) + frame(BIN, b"open", fin=0, key=key(rng))
        probe = FlowRef()
        resume = probe.call(s[:cut])["res"]["resume_off"]
        firsts.append(dict(wire=s[:cut], conn=c))
        seconds.append(dict(wire=s[resume:], conn=c))
    return firsts, seconds


def test_two_calls_queued_on_one_stream(ctx, cuda):
    n = 24
    conns = Conns(cuda, n)
    firsts, seconds = two_queued_calls(cuda, conns, n)
    calls = [Flow(cuda, conns, firsts), Flow(cuda, conns, seconds)]
    outs = [m.expect() for m in calls]                # the second wire was cut at FlowRef's resume_off
    assert sum(1 for o in outs[0] if o["state"]["frame_unread"]) >= 8
    torch.cuda.synchronize()
    for m in calls:
        m.launch(ctx)
    torch.cuda.synchronize()
    for m in calls:
        m.check()
    conns.check()
    for c in range(n):
        assert outs[1][c]["res"]["status"] == 0 and outs[1][c]["state"]["msg"]["open_opcode"] == BIN


def test_graph_capture_and_replay(cuda):
    """One captured call that begins inside a frame, replayed twice: a captured
    copy puts the states back first, so both replays write the same bytes."""
    n = 8
    conns = Conns(cuda, n)
    firsts, seconds = two_queued_calls(cuda, conns, n)
    c = gpu.Ctx(0)                                    # (no reserve: the call has no workspace)
    try:
        run(c, cuda, conns, firsts)
        saved = conns.t.clone()
        m = Flow(cuda, conns, seconds)
        outs = m.expect()
        assert any(o["entries"] and o["entries"][0]["first_frame"] == NONE for o in outs)
        clean = m.arena.clone()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            conns.t.copy_(saved)
            m.launch(c)
        torch.cuda.synchronize()
        for _ in range(2):
            m.arena.copy_(clean)
            g.replay()
            torch.cuda.synchronize()
            m.check()
            conns.check()
    finally:
        torch.cuda.synchronize()
        c.close()


# ------------------------------------------------------------------ 11. MessageFlow
def test_message_flow_returns_the_reference_units(ctx, cuda):
    seeds = [3, 5, 8, 11, 17, 21, 29, 33]
    wires = [random_stream(s)[0] for s in seeds]
    want = [whole(w) for w in wires]
    assert all(s == 0 for _, s, _ in want)
    rng = random.Random(11)
    flow = gpu.MessageFlow(ctx, 8, max_read=700)
    got, pos, feeds = [[] for _ in wires], [0] * 8, 0
    while any(p < len(w) for p, w in zip(pos, wires)):
        reads = {}
        for c, w in enumerate(wires):
            if pos[c] < len(w):
                k = rng.randint(1, 700)
                reads[c] = w[pos[c]:pos[c] + k]
                pos[c] += k
        for c, units in flow.feed(reads).items():
            got[c] += units
        feeds += 1
        assert all(len(p) <= _lib.FWS_MSG_FLOW_MAX_PENDING for p in flow._pending)
    for c in range(8):
        assert got[c] == plain(want[c][0]) and flow.status[c] == 0, c
        st = gpu.read_msg_flow(flow.flows, c)
        assert int(st["msg"]["wire_bytes"]) == len(wires[c]) and int(st["msg"]["n_msgs"]) == len(want[c][0])
        assert int(st["frame_unread"]) == 0
    assert feeds >= 2 and flow.calls == feeds


def test_message_flow_takes_a_1_mib_frame_through_4096_byte_reads(ctx, cuda):
    with pytest.raises(ValueError):
        gpu.MessageMux(ctx, 2, max_read=4096, max_frame=(1 << 20) + 14)
    rng = random.Random(12)
    body = np.random.default_rng(12).integers(0, 256, 1 << 20, dtype=np.uint8).tobytes()
    big = frame(BIN, body, key=key(rng)) + frame(TEXT, b"after", key=key(rng))
    many = mm.tiny_frames(rng, 300) + frame(TEXT, b"after", key=key(rng))
    flow = gpu.MessageFlow(ctx, 2, max_read=4096)
    got = [[], []]
    for at in range(0, len(big), 4096):
        reads = {0: big[at:at + 4096]}
        if at < len(many):
            reads[1] = many[at:at + 4096]
        for c, units in flow.feed(reads).items():
            got[c] += units
    assert got[0] == [(BIN, body, False), (TEXT, b"after", True)]
    assert got[1] == plain(whole(many)[0]) and len(got[1]) == 301
    assert flow.uploaded[0] == len(big) and flow.status == [0, 0]
    assert flow.calls == (len(big) + 4095) // 4096 + 1    # one more for the read with 301 headers
