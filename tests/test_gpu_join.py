"""GPU parity of fws_gpu_join_messages: the messages of many connections that
arrive over several reads put together in device memory, in one launch behind
the decode.

Every test decodes in Multi's arena (test_gpu_msg_flow.Flow, checked there
against FlowRef; the client and the multi call in their own harnesses) and then
joins: the records and the results lie in a second arena that is pre-filled
with a sentinel and compared whole with JoinRef's (join_ref.py; test_join_cpu.py
holds it against FlowRef's units), and so are the state array and the whole of
dev_store -- record / slot 2c is connection c's, the odd ones are guards, a
guard lies in front of the store and one behind it. Where a test says what the
messages are, they are read back from the device through the records. All
comparisons are exact."""
import random

import numpy as np
import pytest
import torch

import client_ref as cr
import join_ref as jr
import test_gpu_client as tc
import test_gpu_msg_carry as cc
import test_gpu_msg_flow as fm
import test_gpu_msg_multi as mm
from flashws_amd import _lib, gpu
from join_ref import DROPPED, IN_DST, IN_STORE, NOWHERE, JoinRef
from test_gpu_msg_carry import BIN, CONT, FILL, GUARD, PING, TEXT, frame, key
from test_gpu_msg_multi import ESZ, align, fill

pytestmark = pytest.mark.gpu

CAPACITY, DECLINED, INVALID, SEQUENCE = (_lib.FWS_ERR_CAPACITY, _lib.FWS_ERR_DECLINED, _lib.FWS_ERR_INVALID,
                                         _lib.FWS_ERR_SEQUENCE)
SMALL, FULL = mm.SMALL, mm.FULL
JSZ, RSZ, SSZ = _lib.JOIN_INFO.itemsize, _lib.JOIN_RESULT.itemsize, _lib.JOIN_STATE.itemsize
FRONT = 256                                               # the guard in front of the store
FORMS = pytest.mark.parametrize("max_len", [SMALL, FULL], ids=["small", "full"])
assert JSZ == ESZ                                         # a record per entry, at the entry's index


class JConns:
    """The join side of a test's connections: fws_join_state records and the
    store on the device, and their references. H: bytes to a half."""

    def __init__(self, cuda, n, H):
        self.n, self.n_dev, self.H, self.stride = n, 2 * n, H, 2 * H
        host = np.full(self.n_dev * SSZ + GUARD, FILL, dtype=np.uint8)
        for c in range(n):
            host[2 * c * SSZ:(2 * c + 1) * SSZ] = 0
        self.states = torch.from_numpy(host).to(cuda)
        self.all = torch.full((FRONT + self.n_dev * self.stride + GUARD,), FILL, dtype=torch.uint8, device=cuda)
        self.store = self.all[FRONT:]
        self.ref = [JoinRef(H, fill=FILL) for _ in range(n)]

    def preset(self, c, **state):
        """A state no call leaves, written by hand."""
        self.ref[c].state = dict(self.ref[c].state, **state)
        rec = np.frombuffer(jr.state_bytes(self.ref[c].state), dtype=np.uint8).copy()
        self.states[2 * c * SSZ:(2 * c + 1) * SSZ] = torch.from_numpy(rec).to(self.states.device)

    def check(self):
        raw = self.states.cpu().numpy().tobytes()
        for c in range(self.n):
            got = np.frombuffer(raw[2 * c * SSZ:(2 * c + 1) * SSZ], dtype=_lib.JOIN_STATE)[0]
            for k in _lib.JOIN_STATE.names:
                assert int(got[k]) == self.ref[c].state[k], ("state", c, k, int(got[k]), self.ref[c].state[k])
            assert raw[(2 * c + 1) * SSZ:(2 * c + 2) * SSZ] == fill * SSZ, ("the guard behind state", c)
        assert raw[self.n_dev * SSZ:] == fill * GUARD
        self.got = got = self.all.cpu().numpy()
        want = np.full(got.size, FILL, dtype=np.uint8)
        for c in range(self.n):
            o = FRONT + 2 * c * self.stride
            want[o:o + self.stride] = np.frombuffer(bytes(self.ref[c].slot), dtype=np.uint8)
        diff = np.nonzero(got != want)[0]
        if diff.size:
            at = int(diff[0]) - FRONT
            assert False, ("the store differs at", at, "slot", at // self.stride, "offset", at % self.stride,
                           "H", self.H, int(got[diff[0]]), int(want[diff[0]]))

    def stored(self, rec):
        """The bytes an IN_STORE record names, from the store as check() fetched it."""
        return self.got[FRONT + rec["off"]:FRONT + rec["off"] + rec["len"]].tobytes()


class Join:
    """One join call over a decode call m (its expect() done). opts[i], per read:
    mres (fields of the read's fws_msg_result) and entries ({j: fields} of its
    fws_msg_info j), overwritten on the device before the call: outputs no decode
    writes, by hand."""

    def __init__(self, cuda, m, jc, opts=None):
        self.m, self.jc, self.n = m, jc, m.n
        self.opts = opts or [{} for _ in range(m.n)]
        off = 0
        self.sec = {}
        for k, sz in (("joined", m.sec["msgs"][1]), ("res", self.n * RSZ)):
            o = align(off + GUARD, 256)
            off = o + sz + GUARD
            self.sec[k] = (o, sz)
        self.host_in = np.full(align(off, 256), FILL, dtype=np.uint8)
        self.arena = torch.from_numpy(self.host_in).to(cuda)
        for i, (r, o) in enumerate(zip(m.reads, self.opts)):
            if "mres" in o:
                self._patch(m.sec["mres"][0] + i * mm.RSZ, _lib.MSG_RESULT, o["mres"])
            for j, fields in o.get("entries", {}).items():
                self._patch(m.sec["msgs"][0] + (r["eb"] + j) * ESZ, _lib.MSG_INFO, fields)

    def _patch(self, at, dtype, fields):
        a = self.m.arena
        rec = np.frombuffer(a[at:at + dtype.itemsize].cpu().numpy().tobytes(), dtype=dtype).copy()
        for k, v in fields.items():
            rec[0][k] = v
        a[at:at + dtype.itemsize] = torch.from_numpy(rec.view(np.uint8).copy()).to(a.device)

    def t(self, k):
        o, sz = self.sec[k]
        return self.arena[o:o + sz + GUARD]

    def expect(self):
        """The references advanced by this call; the arena as it must look afterwards."""
        want = self.host_in.copy()
        self.outs = []
        for i, (r, o) in enumerate(zip(self.m.reads, self.opts)):
            out = self.m.outs[i] if self.m.outs[i] is not None else jr.undecoded(r["expect"])
            if o:
                entries = [dict(e, **o.get("entries", {}).get(j, {})) for j, e in enumerate(out["entries"])]
                out = dict(out, res=dict(out["res"], **o.get("mres", {})), entries=entries)
                if out["res"]["n_msgs"] > len(entries):   # (a count by hand: refused before an entry is read)
                    out["entries"] = entries + [entries[-1]] * (out["res"]["n_msgs"] - len(entries))
            conn = r.get("desc", {}).get("conn", 2 * r["conn"])
            got = self.jc.ref[r["conn"]].call(out, dst_off=r["at"]["dst"], ctl_off=r["at"]["ctl"],
                                              slot_off=conn * self.jc.stride, msg_cap=r["msg_cap"],
                                              dst_cap=r["dst_cap"], ctl_cap=r["ctl_cap"], conn_ok=conn < self.jc.n_dev)
            self.outs.append(got)
            at = self.sec["joined"][0] + r["eb"] * JSZ
            rec = jr.records_bytes(got["records"])
            want[at:at + len(rec)] = np.frombuffer(rec, dtype=np.uint8)
            at = self.sec["res"][0] + i * RSZ
            want[at:at + RSZ] = np.frombuffer(jr.result_bytes(got["res"]), dtype=np.uint8)
        self.want = want
        return self.outs

    def launch(self, ctx, stream=None):
        m, jc = self.m, self.jc
        rc = gpu.join_messages(ctx, m.t("reads"), m.n, m.max_len, m.t("msgs"), m.arena, m.t("mres"), jc.store,
                               jc.stride, self.t("joined"), self.t("res"), jc.states, jc.n_dev, stream=stream)
        assert rc == 0, rc

    def check(self, decode_before=None):
        got = self.got = self.arena.cpu().numpy()
        res = np.frombuffer(got[self.sec["res"][0]:][:self.n * RSZ].tobytes(), dtype=_lib.JOIN_RESULT)
        for i, out in enumerate(self.outs):
            for k in _lib.JOIN_RESULT.names:
                assert int(res[i][k]) == out["res"][k], ("result", i, k, int(res[i][k]), out["res"][k])
            at = self.sec["joined"][0] + self.m.reads[i]["eb"] * JSZ
            recs = np.frombuffer(got[at:at + len(out["records"]) * JSZ].tobytes(), dtype=_lib.JOIN_INFO)
            for j, want in enumerate(out["records"]):
                for k in _lib.JOIN_INFO.names:
                    assert int(recs[j][k]) == want[k], ("record", i, j, k, int(recs[j][k]), want[k])
        diff = np.nonzero(got != self.want)[0]
        assert diff.size == 0, ("the arena differs at", int(diff[0]), self.sec)
        if decode_before is not None:                 # the call only reads what the decode wrote
            assert self.m.arena.cpu().numpy().tobytes() == decode_before, "the decode's arena was modified"

    def units(self, i):
        """Read i's units from the device, through the records: (opcode, bytes or None, utf8_ok)."""
        out = []
        for rec in self.outs[i]["records"]:
            if rec["where"] == IN_STORE:
                body = self.jc.stored(rec)
            elif rec["where"] == NOWHERE:
                body = None
            else:                                     # dev_dst and dev_ctl are the decode's arena
                body = self.m.got[rec["off"]:rec["off"] + rec["len"]].tobytes()
            out.append((rec["opcode"], body, rec["utf8_ok"]))
        return out


def join(ctx, cuda, m, jc, opts=None):
    """One join call over the decode call m, checked in full."""
    jn = Join(cuda, m, jc, opts)
    before = m.arena.cpu().numpy().tobytes()
    jn.expect()
    jn.launch(ctx)
    torch.cuda.synchronize()
    jn.check(before)
    jc.check()
    m.conns.check()                                   # the decode's states: never written
    return jn


def step(ctx, cuda, conns, jc, reads, max_len=None, opts=None, run=fm.run):
    """decode + join, both checked in full: (the decode's outputs, the join call)."""
    outs, m, _ = run(ctx, cuda, conns, reads, max_len)
    return outs, join(ctx, cuda, m, jc, opts)


def feed_all(ctx, cuda, conns, jc, streams, cuts, max_len=None, run=fm.run, order=None, **caps):
    """fm.feed_all with the join behind every decode: connection c gets
    streams[c] cut at cuts[c], call k serves every connection (in `order`) up to
    its k-th cut. Returns (the calls, the units per connection as the device
    holds them)."""
    n = len(streams)
    order = list(order or range(n))
    ends = [sorted(set(cs)) + [len(s)] for s, cs in zip(streams, cuts)]
    pos, calls, units = [0] * n, [], [[] for _ in range(n)]
    for k in range(max(map(len, ends))):
        reads = [dict(wire=streams[c][pos[c]:ends[c][min(k, len(ends[c]) - 1)]], conn=c, **caps) for c in order]
        outs, jn = step(ctx, cuda, conns, jc, reads, max_len, run=run)
        for i, c in enumerate(order):
            pos[c] += outs[i]["res"]["resume_off"]
            units[c] += jn.units(i)
        calls.append((outs, jn))
    assert pos == [len(s) for s in streams]
    return calls, units


def plain(units):
    """FlowRef's units without their frame counts."""
    return [(op, body, ok) for op, body, ok, *_ in units]


def count(calls, where):
    return sum(1 for _, jn in calls for o in jn.outs for r in o["records"] if r["where"] == where)


def one_frame(rng, n, op=BIN):
    body = cc.payload(rng, n)
    return frame(op, body, key=key(rng)), body


# ------------------------------------------------------------------ 1. alignment
FILLS = tuple(range(18)) + (31, 32, 33)
LENS = (0, 1, 2, 3, 4, 15, 16, 17, 31, 32, 33, 47)


@FORMS
def test_fill_and_part_length_sweep_in_both_halves(ctx, cuda, max_len):
    """Two messages in a row, each a frame of f + p + q bytes cut after f and
    after f + p (p = 0: in two): the parts are appended at fill 0, f and f + p,
    the first message in half 0 and the second in half 1, whose first part
    arrives in the read that completes the first."""
    rng = random.Random(1)
    streams, cuts, want = [], [], []
    for f in FILLS:
        for j, p in enumerate(LENS):
            q = LENS[(j + f) % len(LENS)] + 1              # (the last part holds a byte: the frame ends there)
            (a, body_a), (b, body_b) = one_frame(rng, f + p + q), one_frame(rng, f + p + q)
            assert len(a) == 6 + f + p + q               # (the 7-bit length form)
            streams.append(a + b)
            cuts.append([6 + f, 6 + f + p, len(a) + 6 + f, len(a) + 6 + f + p])
            want.append([(BIN, body_a, 0), (BIN, body_b, 0)])
    n = len(streams)
    conns, jc = fm.Conns(cuda, n), JConns(cuda, n, 128)
    calls, units = feed_all(ctx, cuda, conns, jc, streams, cuts, max_len)
    assert units == want
    assert count(calls, IN_STORE) == 2 * n and count(calls, NOWHERE) == 0
    offs = {r["off"] % jc.stride for _, jn in calls for o in jn.outs for r in o["records"]}
    assert offs == {0, 128}                               # both halves
    # a message opened with 0 bytes present; an empty read
    assert any(o["res"]["open_opcode"] and o["res"]["open_len"] == 0 for o in calls[0][0])
    assert any(len(r["wire"]) == 0 for r in calls[-1][1].m.reads)


def test_open_off_sweep(ctx, cuda):
    """The open part's source offset over every residue of 16: a whole message
    of k bytes in front of it."""
    rng = random.Random(2)
    streams, cuts, want = [], [], []
    for k in range(32):
        for p in (1, 15, 16, 17, 33, 47):
            body_f = cc.random_text(rng, k) if k % 2 else cc.payload(rng, k)
            front = frame(TEXT if k % 2 else BIN, body_f, key=key(rng))
            msg, body = one_frame(rng, p + 5)
            streams.append(front + msg)
            cuts.append([len(front) + 6 + p])
            want.append([(TEXT if k % 2 else BIN, body_f, k % 2), (BIN, body, 0)])
    n = len(streams)
    conns, jc = fm.Conns(cuda, n), JConns(cuda, n, 64)
    calls, units = feed_all(ctx, cuda, conns, jc, streams, cuts)
    assert units == want
    assert {o["res"]["open_off"] & 15 for o in calls[0][0]} == set(range(16))
    assert count(calls, IN_STORE) == n and count(calls, IN_DST) == n


# ------------------------------------------------------------------ 2. the half boundary
@pytest.mark.parametrize("H", [16, 48])
def test_half_boundary_and_the_message_after_a_drop(ctx, cuda, H):
    """fill + len = H - 1 and H are kept, H + 1 is dropped at the CONTINUED
    entry, H + 2 in three parts already at an open part; the next message of the
    connection is joined as if nothing had happened."""
    rng = random.Random(3 + H)
    streams, cuts, want, totals = [], [], [], []
    for total in (H - 1, H, H + 1, H + 2):
        for f in sorted({0, 1, 15, 16, 17, H - 1} & set(range(total))):
            for three in ((False, True) if total <= H + 1 else (True,)):
                msg, body = one_frame(rng, total)
                nxt, body_n = one_frame(rng, H - 3)
                streams.append(msg + nxt)
                # in three: the last part is one byte
                cs = [6 + f] + ([6 + total - 1] if three and f < total - 1 else [])
                cuts.append(cs + [len(msg) + 6 + 2])
                want.append([(BIN, body if total <= H else None, 0), (BIN, body_n, 0)])
                totals.append(total)
    n = len(streams)
    conns, jc = fm.Conns(cuda, n), JConns(cuda, n, H)
    calls, units = feed_all(ctx, cuda, conns, jc, streams, cuts)
    assert units == want
    drops = [r for _, jn in calls for o in jn.outs for r in o["records"] if r["where"] == NOWHERE]
    assert len(drops) == totals.count(H + 1) + totals.count(H + 2)
    assert all(r["len"] in (H + 1, H + 2) and r["flags"] == DROPPED and r["off"] == 0 for r in drops)
    assert any(o["res"]["dropped"] for _, jn in calls for o in jn.outs)        # dropped at an open part
    for c in range(n):                                    # a drop does not toggle the half
        off = [r["off"] % jc.stride for _, jn in calls for i, o in enumerate(jn.outs) if jn.m.reads[i]["conn"] == c
               for r in o["records"] if r["where"] == IN_STORE]
        assert off == ([0, H] if totals[c] <= H else [0]), c


# ------------------------------------------------------------------ 3. sequences
def test_sequences(ctx, cuda):
    rng = random.Random(4)
    m = []                                               # BIN, TEXT, BIN, TEXT of 40, 47, 54 and 61 bytes
    for j in range(4):
        body = cc.random_text(rng, 40 + 7 * j) if j % 2 else cc.payload(rng, 40 + 7 * j)
        m.append((frame(TEXT if j % 2 else BIN, body, key=key(rng)), body))
    text = cc.random_text(rng, 90)
    big, big_body = one_frame(rng, 3000)
    whole_one, whole_body = one_frame(rng, 21)
    streams = [
        # four messages in a row that each span reads: the halves alternate
        b"".join(w for w, _ in m),
        # a message over three reads, the middle one a PING only: it adds 0 bytes
        frame(TEXT, text[:50], fin=0, key=key(rng)) + frame(PING, b"still there", key=key(rng)) +
        frame(CONT, text[50:], fin=1, key=key(rng)),
        # a frame over three reads, the middle one all payload (n_frames = 0)
        big,
        # a read that completes a joined message, holds a whole one and opens a third
        m[0][0] + whole_one + m[1][0],
        # a message opened with 0 bytes present: the read ends behind its header
        whole_one + m[2][0],
        # a last part of 0 bytes: an empty FIN continuation alone in its read
        frame(BIN, whole_body, fin=0, key=key(rng)) + frame(CONT, b"", fin=1, key=key(rng)),
    ]
    at = [0]
    for w, _ in m:
        at.append(at[-1] + len(w))
    ping_at = len(frame(TEXT, text[:50], fin=0, key=0))
    cuts = [[at[j] + 6 + 11 + j for j in range(4)],
            [ping_at, ping_at + 6 + 11],
            [700, 2100],
            [20, len(m[0][0]) + len(whole_one) + 9],
            [len(whole_one) + 6],
            [len(whole_one)]]
    conns, jc = fm.Conns(cuda, 6), JConns(cuda, 6, 4096)
    calls, units = feed_all(ctx, cuda, conns, jc, streams, cuts)
    assert units[0] == [(TEXT if j % 2 else BIN, body, j % 2) for j, (_, body) in enumerate(m)]
    assert units[1] == [(PING, b"still there", 0), (TEXT, text, 1)]
    assert units[2] == [(BIN, big_body, 0)]
    assert units[3] == [(BIN, m[0][1], 0), (BIN, whole_body, 0), (TEXT, m[1][1], 1)]
    assert units[4] == [(BIN, whole_body, 0), (BIN, m[2][1], 0)]
    assert units[5] == [(BIN, whole_body, 0)]
    stored = [[r["off"] % jc.stride for _, jn in calls for i, o in enumerate(jn.outs) if jn.m.reads[i]["conn"] == c
               for r in o["records"] if r["where"] == IN_STORE] for c in range(6)]
    assert stored == [[0, 4096, 0, 4096], [0], [0], [0, 4096], [0], [0]]
    assert calls[1][0][1]["res"]["open_len"] == 0 and calls[1][0][1]["res"]["n_msgs"] == 1     # the PING's read
    assert calls[1][0][2]["dres"]["n_frames"] == 0 and calls[1][1].outs[2]["res"]["copied"] == 1400
    recs = calls[1][1].outs[3]["records"]                # completed, whole, and a third opened: one read
    assert [r["where"] for r in recs] == [IN_STORE, IN_DST] and calls[1][1].outs[3]["res"]["open_opcode"] == TEXT
    assert calls[0][0][4]["res"]["open_len"] == 0 and calls[0][1].outs[4]["res"]["open_opcode"] == BIN
    assert calls[1][0][5]["entries"][0]["len"] == 0 and calls[1][1].outs[5]["res"]["copied"] == 0


# ------------------------------------------------------------------ 4. size
def test_a_20_kib_part_and_a_300_kib_message(ctx, cuda):
    rng = np.random.default_rng(5)
    r = random.Random(5)
    body_a = rng.integers(0, 256, (20 << 10) + 333, dtype=np.uint8).tobytes()
    body_b = rng.integers(0, 256, 300 << 10, dtype=np.uint8).tobytes()
    streams = [frame(TEXT, b"front", key=key(r)) + frame(BIN, body_a, key=key(r)), frame(BIN, body_b, key=key(r))]
    cuts = [[11 + 8 + (20 << 10)], [100 << 10, 228 << 10]]        # (reads of at most 128 KiB)
    conns, jc = fm.Conns(cuda, 2), JConns(cuda, 2, 320 << 10)
    calls, units = feed_all(ctx, cuda, conns, jc, streams, cuts, FULL)
    assert units == [[(TEXT, b"front", 1), (BIN, body_a, 0)], [(BIN, body_b, 0)]]
    assert calls[0][1].outs[0]["res"]["copied"] == 20 << 10 and calls[0][1].m.max_len == FULL
    assert [jn.outs[1]["res"]["copied"] for _, jn in calls] == [(100 << 10) - 14, 128 << 10, (72 << 10) + 14]


# ------------------------------------------------------------------ 5. statuses
def test_a_sequencing_error_with_a_valid_prefix_is_joined(ctx, cuda):
    rng = random.Random(6)
    first, body = one_frame(rng, 30)
    ok_msg, ok_body = one_frame(rng, 9)
    opener = frame(BIN, b"opened", fin=0, key=key(rng))
    conns, jc = fm.Conns(cuda, 1), JConns(cuda, 1, 64)
    step(ctx, cuda, conns, jc, [dict(wire=first[:20], conn=0)])
    outs, jn = step(ctx, cuda, conns, jc, [dict(wire=first[20:] + ok_msg + opener + frame(TEXT, b"new", key=key(rng)),
                                                conn=0)])
    assert outs[0]["res"]["status"] == SEQUENCE and outs[0]["res"]["n_msgs"] == 2
    assert jn.units(0) == [(BIN, body, 0), (BIN, ok_body, 0)]
    assert jn.outs[0]["res"] == dict(status=0, n_joined=2, copied=16 + 6, open_opcode=BIN, dropped=0, reserved=0)
    assert jc.ref[0].state == dict(open_opcode=BIN, half=1, dropped=0, reserved0=0, open_bytes=6, fill=6)


def test_nothing_to_do_leaves_state_and_store_untouched(ctx, cuda):
    rng = random.Random(7)
    msg, body = one_frame(rng, 50)
    conns, jc = fm.Conns(cuda, 4), JConns(cuda, 4, 64)
    step(ctx, cuda, conns, jc, [dict(wire=msg[:30], conn=c) for c in range(4)])
    states, store = jc.states.clone(), jc.all.clone()
    rest = msg[30:]
    reads = [dict(wire=rest, conn=0, dst_cap=16),                              # an undelivered decode
             dict(wire=rest + bytes(40), conn=1, expect=DECLINED),             # longer than max_len
             dict(wire=rest, conn=2, expect=INVALID, desc=dict(conn=jc.n_dev)),   # conn >= n_conns: refused
             dict(wire=b"", conn=3)]                                           # an empty read
    outs, jn = step(ctx, cuda, conns, jc, reads, max_len=len(rest))
    assert outs[0]["res"]["status"] == CAPACITY and outs[0]["res"]["resume_off"] == 0
    want = dict(status=0, n_joined=0, copied=0, open_opcode=BIN, dropped=0, reserved=0)
    assert [o["res"] for o in jn.outs] == [want, want, dict(want, status=INVALID, open_opcode=0), want]
    assert torch.equal(jc.states, states) and torch.equal(jc.all, store)
    # the same bytes again, delivered: the messages complete
    outs, jn = step(ctx, cuda, conns, jc, [dict(wire=rest, conn=c) for c in (0, 1, 3)])
    assert [jn.units(i) for i in range(3)] == [[(BIN, body, 0)]] * 3


def test_out_of_step_reads_are_refused(ctx, cuda):
    """Each refusal by hand: the decode's output is rewritten on the device
    before the join. Only the result is written."""
    rng = random.Random(8)
    msg, _ = one_frame(rng, 50)
    whole_msg, _ = one_frame(rng, 12)
    n = 10
    conns, jc = fm.Conns(cuda, n), JConns(cuda, n, 64)
    # connections 0-4 and 9 have a message open, 5-8 have none
    step(ctx, cuda, conns, jc, [dict(wire=msg[:30], conn=c) for c in (0, 1, 2, 3, 4, 9)])
    jc.preset(9, open_opcode=3)
    states, store = jc.states.clone(), jc.all.clone()
    rest = msg[30:]
    big = _lib.FWS_MSG_MULTI_MAX_READ + 1
    reads = [dict(wire=rest + whole_msg, conn=0), dict(wire=rest, conn=1), dict(wire=rest[:5], conn=2),
             dict(wire=rest[:5], conn=3), dict(wire=rest[:5], conn=4),
             dict(wire=whole_msg, conn=5), dict(wire=whole_msg, conn=6), dict(wire=msg[:30], conn=7),
             dict(wire=whole_msg, conn=8, msg_cap=300), dict(wire=rest, conn=9)]
    opts = [dict(entries={1: dict(flags=1)}),            # a CONTINUED entry that is not the first data entry
            dict(entries={0: dict(flags=0)}),            # a message open, a data entry, no CONTINUED entry
            dict(mres=dict(open_opcode=TEXT)),           # a message open, another one's open part
            dict(mres=dict(open_opcode=0)),              # a message open, no open part
            dict(mres=dict(open_len=big)),               # an open part no read holds
            dict(entries={0: dict(flags=1)}),            # a CONTINUED entry, nothing open
            dict(entries={0: dict(len=big)}),            # a data entry no read holds
            dict(mres=dict(open_len=big)),
            dict(mres=dict(n_msgs=258)),                 # more entries than a decode writes
            {}]                                          # the state's open_opcode is none of 0, 1, 2
    outs, m, _ = fm.run(ctx, cuda, conns, reads)
    jn = join(ctx, cuda, m, jc, opts)
    refused = dict(status=INVALID, n_joined=0, copied=0, open_opcode=0, dropped=0, reserved=0)
    assert [o["res"] for o in jn.outs] == [refused] * n
    assert torch.equal(jc.states, states) and torch.equal(jc.all, store)


# ------------------------------------------------------------------ 6. isolation
@FORMS
def test_64_connections_permuted(ctx, cuda, max_len):
    made = [cc.random_cuts(s) for s in range(64)]
    streams, cuts = [w for w, _ in made], [cs for _, cs in made]
    order = list(range(64))
    random.Random(9).shuffle(order)
    # a half of 256 bytes: most joined messages are kept, some are dropped
    conns, jc = fm.Conns(cuda, 64), JConns(cuda, 64, 256)
    calls, units = feed_all(ctx, cuda, conns, jc, streams, cuts, max_len, order=order)
    dropped = 0
    for c in range(64):
        want = plain(cc.whole(streams[c])[0])
        assert len(units[c]) == len(want), c
        for got, w in zip(units[c], want):
            assert got == w or (got[1] is None and got[0] == w[0] and got[2] == w[2] and len(w[1]) > 256), c
            dropped += got[1] is None
    kept = count(calls, IN_STORE)
    assert kept >= 40 and dropped >= 10 and dropped == count(calls, NOWHERE), (kept, dropped)


# ------------------------------------------------------------------ 7. chaining
def test_decode_join_decode_join_queued_on_one_stream(ctx, cuda):
    n = 24
    conns, jc = fm.Conns(cuda, n), JConns(cuda, n, 512)
    firsts, seconds = fm.two_queued_calls(cuda, conns, n)
    decodes = [fm.Flow(cuda, conns, firsts), fm.Flow(cuda, conns, seconds)]
    for m in decodes:
        m.expect()
    joins = [Join(cuda, m, jc) for m in decodes]
    for j in joins:
        j.expect()
    torch.cuda.synchronize()
    for m, j in zip(decodes, joins):                      # nothing between the four launches
        m.launch(ctx)
        j.launch(ctx)
    torch.cuda.synchronize()
    for m, j in zip(decodes, joins):
        m.check()
        j.check()
    jc.check()
    conns.check()
    spanning = [c for c in range(n) if c % 3]             # the first read ends inside the TEXT frame
    assert len(spanning) == 16
    for c in spanning:
        rec = joins[1].outs[c]["records"][0]
        op, body, ok, _ = decodes[1].outs[c]["units"][0]      # the TEXT message of 90 + 7 c bytes
        assert (op, len(body), ok) == (TEXT, 90 + 7 * c, 1)
        assert rec["where"] == IN_STORE and jc.stored(rec) == body and rec["utf8_ok"] == 1, c
    assert all(o["res"]["open_opcode"] == BIN for o in joins[1].outs)


# ------------------------------------------------------------------ 8. a slot past 4 GiB
def test_a_slot_that_starts_past_4_gib(ctx, cuda):
    """store_stride a little over 2 GiB and conn 2: every offset of the slot needs
    more than 32 bits. The store is not held whole: windows of it are
    sentinel-filled and compared -- the start of the store and of slot 1, where a
    truncated offset would land, and both halves of slot 2 with what lies in
    front of them."""
    stride, WIN = (2 << 30) + 64, 64 << 10
    H = stride // 2
    rng = random.Random(10)
    a, body_a = one_frame(rng, 5000)
    b, body_b = one_frame(rng, 777)
    stream = a + b
    conns = fm.Conns(cuda, 2)
    ref = JoinRef(H, fill=FILL, window=WIN)
    states = torch.zeros(4 * SSZ, dtype=torch.uint8, device=cuda)
    store = torch.empty(3 * stride, dtype=torch.uint8, device=cuda)
    windows = [0, stride - WIN, stride, 2 * stride - WIN, 2 * stride, 2 * stride + H - WIN, 2 * stride + H]
    for w in windows:
        store[w:w + WIN] = FILL
    pos, got = 0, []
    for end in (2000, len(a) + 100, len(stream)):
        outs, m, _ = fm.run(ctx, cuda, conns, [dict(wire=stream[pos:end], conn=1)])
        pos += outs[0]["res"]["resume_off"]
        r = m.reads[0]
        want = ref.call(outs[0], dst_off=r["at"]["dst"], ctl_off=r["at"]["ctl"], slot_off=2 * stride)
        joined = torch.full((r["msg_cap"] * JSZ + GUARD,), FILL, dtype=torch.uint8, device=cuda)
        res = torch.full((RSZ + GUARD,), FILL, dtype=torch.uint8, device=cuda)
        rc = gpu.join_messages(ctx, m.t("reads"), 1, m.max_len, m.t("msgs"), m.arena, m.t("mres"),
                               store, stride, joined, res, states, 4)
        assert rc == 0
        torch.cuda.synchronize()
        assert res.cpu().numpy().tobytes() == jr.result_bytes(want["res"]) + fill * GUARD
        rec = jr.records_bytes(want["records"])
        assert joined.cpu().numpy().tobytes() == rec + fill * (r["msg_cap"] * JSZ + GUARD - len(rec))
        for x in want["records"]:
            assert x["where"] == IN_STORE and x["off"] >= 1 << 32
            got.append((x["opcode"], store[x["off"]:x["off"] + x["len"]].cpu().numpy().tobytes(), x["utf8_ok"]))
    assert got == [(BIN, body_a, 0), (BIN, body_b, 0)] and got[1][1] == ref.stored(want["records"][0], 2 * stride)
    assert [x["off"] for x in want["records"]] == [2 * stride + H]
    for w in windows:
        have = store[w:w + WIN].cpu().numpy().tobytes()
        half = {2 * stride: 0, 2 * stride + H: 1}.get(w)
        assert have == (fill * WIN if half is None else bytes(ref.slot[half * WIN:(half + 1) * WIN])), w
    st = np.frombuffer(states.cpu().numpy().tobytes(), dtype=_lib.JOIN_STATE)
    assert st[2].tobytes() == jr.state_bytes(ref.state) and st[[0, 1, 3]].tobytes() == bytes(3 * SSZ)


# ------------------------------------------------------------------ 9. roles and forms
@FORMS
def test_after_the_client_decode(ctx, cuda, max_len):
    made = [cr.random_server_stream(seed, edges=(0, 125, 126)) for seed in range(20)]
    streams = [w for w, _, _ in made]
    cuts = [cr.random_cuts(seed, w, spans, 2, 6) for seed, (w, spans, _) in enumerate(made)]
    conns, jc = tc.Conns(cuda, 20), JConns(cuda, 20, 16 << 10)
    calls, units = feed_all(ctx, cuda, conns, jc, streams, cuts, max_len, run=tc.run)
    for c, (_, _, want) in enumerate(made):
        assert [(op, body) for op, body, _ in units[c]] == want, c
        assert [u[2] for u in units[c]] == [u[2] for u in conns.units[c]], c
    assert count(calls, IN_STORE) >= 10 and count(calls, NOWHERE) == 0


@FORMS
def test_after_the_multi_decode(ctx, cuda, max_len):
    made = [cc.random_cuts(s) for s in range(20)]
    streams, cuts = [w for w, _ in made], [cs for _, cs in made]
    conns, jc = mm.Conns(cuda, 20), JConns(cuda, 20, 4096)
    calls, units = feed_all(ctx, cuda, conns, jc, streams, cuts, max_len, run=mm.run)
    for c in range(20):
        assert units[c] == plain(cc.whole(streams[c])[0]), c
    assert count(calls, IN_STORE) >= 20 and count(calls, NOWHERE) == 0


# ------------------------------------------------------------------ 10. MessageJoiner
def pump(feed, wires, rng, max_read):
    """The wires fed in random reads of up to max_read bytes: the units per connection."""
    got, pos = [[] for _ in wires], [0] * len(wires)
    while any(p < len(w) for p, w in zip(pos, wires)):
        reads = {}
        for c, w in enumerate(wires):
            if pos[c] < len(w):
                k = rng.randint(1, max_read)
                reads[c] = w[pos[c]:pos[c] + k]
                pos[c] += k
        for c, units in feed(reads).items():
            got[c] += units
    return got


def test_message_joiner_equals_message_flow(ctx, cuda):
    seeds = [3, 5, 8, 11, 17, 21, 29, 33]
    wires = [cc.random_stream(s)[0] for s in seeds]
    wires[7] += mm.tiny_frames(random.Random(11), 300)    # more headers than one call takes: the retry is joined too
    want = pump(gpu.MessageFlow(ctx, 8, max_read=300).feed, wires, random.Random(12), 300)
    for c, w in enumerate(wires):
        assert want[c] == plain(cc.whole(w)[0]), c
    flow = gpu.MessageFlow(ctx, 8, max_read=300)
    joiner = gpu.MessageJoiner(flow, max_message=2048)
    got = pump(joiner.feed, wires, random.Random(12), 300)
    assert got == want
    assert flow._parts == [[] for _ in range(8)] and joiner.store_copies >= 8 and joiner.calls == flow.calls
    for c in range(8):
        st = gpu.read_join_state(joiner.states, c)
        assert int(st["open_opcode"]) == 0 and int(st["fill"]) == 0 and flow.status[c] == 0
    # a half too small for some: those come back as (opcode, None, utf8_ok), every other one as before
    flow = gpu.MessageFlow(ctx, 8, max_read=300)
    small = gpu.MessageJoiner(flow, max_message=200)
    assert small.half == 208 and small.stride == 416
    got = pump(small.feed, wires, random.Random(12), 300)
    dropped = 0
    for c in range(8):
        assert len(got[c]) == len(want[c])
        for g, w in zip(got[c], want[c]):
            assert g == w or (g == (w[0], None, w[2]) and len(w[1]) > 208), c
            dropped += g[1] is None
    assert dropped >= 5 and flow._parts == [[] for _ in range(8)]


def test_message_joiner_with_a_strict_responder(ctx, cuda):
    """A responder attached to the joiner answers what the joiner decodes: the
    units are MessageFlow's, the replies those of a responder on a plain flow."""
    seeds = [2, 4, 6, 9]
    wires = [cc.random_stream(s)[0] for s in seeds]
    flags = _lib.FWS_REPLY_CONTROL | _lib.FWS_REPLY_ECHO

    def run(with_joiner):
        flow = gpu.MessageFlow(ctx, 4, max_read=500)
        top = gpu.MessageJoiner(flow, max_message=4096) if with_joiner else flow
        resp = gpu.MessageResponder(top, flags, strict=True, max_message=4096)
        replies = [b""] * 4

        def feed(reads):
            units, rep = resp.feed(reads)
            for c, b in rep.items():
                replies[c] += b
            return units

        alive = [True] * 4
        got, pos, rng = [[] for _ in wires], [0] * 4, random.Random(13)
        while any(alive[c] and pos[c] < len(w) for c, w in enumerate(wires)):
            reads = {}
            for c, w in enumerate(wires):
                if alive[c] and pos[c] < len(w):
                    k = rng.randint(1, 500)
                    reads[c] = w[pos[c]:pos[c] + k]
                    pos[c] += k
            for c, units in feed(reads).items():
                got[c] += units
            for c in resp.failed:                         # (a TEXT message that is not UTF-8: 1007, and no more reads)
                alive[c] = False
        return got, replies, dict(resp.failed), flow, top

    want, want_replies, want_failed, _, _ = run(False)
    got, replies, failed, flow, joiner = run(True)
    assert got == want and replies == want_replies and failed == want_failed
    assert sum(map(len, got)) > 50 and any(replies) and flow._parts == [[] for _ in range(4)]
    assert joiner.store_copies >= 4 and flow._queued is None and joiner._queued is None
