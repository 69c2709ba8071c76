"""GPU parity of fws_gpu_reply_messages_strict: the reply call that fails a
connection on the device -- the first failing item of a read answered with a
CLOSE carrying 1002, 1007 or 1009, nothing behind it.

As test_gpu_reply.py: a flow decode in Multi's arena, then the strict reply
into a sentinel-filled arena compared whole against StrictRef (fail_ref.py) --
regions, guards, records and results exactly, the fws_tx_conn and
fws_reply_state arrays with their guard records, and the decode's own state
array once more after the reply, which must not have touched it. Both kernel
forms unless noted. All comparisons are exact."""
import random
import struct

import numpy as np
import pytest
import torch

import fail_ref
import reply_ref as rr
import test_gpu_msg_carry as cc
import test_gpu_msg_flow as fm
import test_gpu_msg_multi as mm
import test_gpu_reply as rp
import utf8_corpus as uc
from fail_ref import StrictRef
from flashws_amd import _lib, gpu
from reply_ref import CONTROL, ECHO
from test_gpu_msg_carry import BIN, CLOSE, CONT, FILL, PING, PONG, TEXT, key
from test_reply_strict_cpu import CASES
from wsframes import frame

pytestmark = pytest.mark.gpu

CAPACITY, INVALID, SEQUENCE = _lib.FWS_ERR_CAPACITY, _lib.FWS_ERR_INVALID, _lib.FWS_ERR_SEQUENCE
SMALL, FULL, BOTH, FORMS = rp.SMALL, rp.FULL, rp.BOTH, rp.FORMS
FAIL = {1002: bytes.fromhex("880203EA"), 1007: bytes.fromhex("880203EF"), 1009: bytes.fromhex("880203F1")}
K = 0x5A3C9F17


class SConns(rp.RConns):
    """RConns whose references are StrictRef; limit is the calls' max_message_bytes."""

    def __init__(self, cuda, n, flags=BOTH, limit=0):
        super().__init__(cuda, n, flags)
        self.limit = limit
        self.ref = [StrictRef(flags, limit) for _ in range(n)]


class Strict(rp.Reply):
    """Reply launched as the strict call over the decode call's own state array."""

    def launch(self, ctx, stream=None):
        m = self.m
        stride = fm.SSZ if isinstance(m, fm.Flow) else mm.CSZ
        assert m.conns.t.numel() >= m.conns.n_dev * stride
        rc = gpu.reply_messages_strict(ctx, m.t("reads"), m.n, m.max_len, m.t("msgs"), m.arena, m.arena, m.t("mres"),
                                       m.conns.t, stride, self.rc.limit, self.t("regions"), self.arena,
                                       self.t("frames"), self.t("res"), self.rc.tx, self.rc.st, self.rc.n_dev,
                                       self.flags, stream=stream)
        assert rc == 0, rc


def strict(ctx, cuda, m, rc, opts=None, flags=None):
    sp = Strict(cuda, m, rc, opts, flags)
    sp.expect()
    sp.launch(ctx)
    torch.cuda.synchronize()
    sp.check()
    rc.check()
    m.conns.check()                                   # the decode's states: read, never written
    return sp


def step(ctx, cuda, conns, rc, reads, max_len=None, opts=None):
    outs, m, _ = fm.run(ctx, cuda, conns, reads, max_len)
    return outs, strict(ctx, cuda, m, rc, opts)


def rounds(ctx, cuda, streams, flags=BOTH, limit=0, max_len=None):
    """Connection c gets streams[c], a list of reads, round by round (what a
    call left unconsumed goes in front of the next read). Returns (rc, the
    strict calls)."""
    n = len(streams)
    conns, rc = fm.Conns(cuda, n), SConns(cuda, n, flags, limit)
    pending, calls = [b""] * n, []
    for k in range(max(map(len, streams))):
        live = [c for c in range(n) if k < len(streams[c])]
        reads = [dict(wire=pending[c] + streams[c][k], conn=c) for c in live]
        outs, sp = step(ctx, cuda, conns, rc, reads, max_len)
        for c, out in zip(live, outs):
            pending[c] = (pending[c] + streams[c][k])[out["res"]["resume_off"]:]
        calls.append(sp)
    return rc, calls


def fail_codes(rc):
    """fail_code of every connection, from the device (the odd records are guards)."""
    raw = np.frombuffer(rc.st.cpu().numpy()[:rc.n_dev * rp.SSZ].tobytes(), dtype=_lib.REPLY_STATE)
    return [int(x) for x in raw["fail_code"][::2]]


# ------------------------------------------------------------------ 1. the case list
@FORMS
def test_the_case_list(ctx, cuda, max_len):
    groups = {}
    for case in CASES:
        groups.setdefault((case[2], case[3]), []).append(case)
    assert len(groups) >= 4
    for (flags, limit), cases in groups.items():
        rc, calls = rounds(ctx, cuda, [c[1] for c in cases], flags, limit, max_len)
        assert fail_codes(rc) == [c[5] for c in cases]
        for i, (name, reads, _, _, want, code) in enumerate(cases):
            assert rc.ref[i].wire == bytes.fromhex(want), name
            if len(reads) == 1:
                assert calls[0].region(i) == bytes.fromhex(want), name


# ------------------------------------------------------------------ 2. non-failing streams equal the plain call
@FORMS
@pytest.mark.parametrize("flags", [BOTH, ECHO], ids=["both", "echo"])
def test_non_failing_streams_equal_the_plain_call(ctx, cuda, flags, max_len):
    stream = rp.closing_stream()
    L = len(stream)
    n = L + 1
    conns, plain, rc = fm.Conns(cuda, n), rp.RConns(cuda, n, flags), SConns(cuda, n, flags)
    pos = [0] * n
    for ends in ([c for c in range(n)], [L] * n):
        outs, m, _ = fm.run(ctx, cuda, conns, [dict(wire=stream[pos[c]:ends[c]], conn=c) for c in range(n)], max_len)
        a = rp.reply(ctx, cuda, m, plain)
        b = strict(ctx, cuda, m, rc)
        assert torch.equal(a.arena, b.arena)
        assert torch.equal(plain.tx, rc.tx) and torch.equal(plain.st, rc.st)
        for c, out in enumerate(outs):
            pos[c] += out["res"]["resume_off"]
    assert pos == [L] * n and fail_codes(rc) == [0] * n


# ------------------------------------------------------------------ 3. the CLOSE code sweep
@FORMS
def test_close_code_sweep(ctx, cuda, max_len):
    codes = list(range(5001)) + [65535]
    reads = [dict(wire=frame(CLOSE, struct.pack(">H", c), key=(K + 0x01000193 * c) & 0xFFFFFFFF), conn=i, cap=2, msg_cap=2,
                  dst_cap=16, ctl_cap=16) for i, c in enumerate(codes)]
    assert all(len(r["wire"]) == 8 for r in reads)
    conns, rc = fm.Conns(cuda, len(codes)), SConns(cuda, len(codes))
    _, sp = step(ctx, cuda, conns, rc, reads, max_len)
    allowed = set(range(1000, 1004)) | set(range(1007, 1015)) | set(range(3000, 5000))
    assert fail_codes(rc) == [0 if c in allowed else 1002 for c in codes]
    for i, c in enumerate(codes):
        assert sp.region(i) == (b"\x88\x02" + struct.pack(">H", c) if c in allowed else FAIL[1002]), c
        assert rc.ref[i].state["close_code"] == c


# ------------------------------------------------------------------ 4. CLOSE reasons from the conformance corpus
SLOT = 160                                                # a read's slice of ctl and of the output


def reason_corpus():
    """(data[n, 123], lens[n], ok[n], cut[n]): the reasons, Python's verdicts, and
    which end in a sequence of Table 3-7 or a proper prefix of one (cut by the end)."""
    rows, cut = [], []
    for seq in uc.seq_s():
        for before, after in ((0, 0), (5, 0), (0, 5), (118, 0), (59, 59), (0, 118)):
            rows.append(uc.s_case(before, seq, after)[0])
            cut.append(after == 0 and (seq in uc.seq_v() or seq in uc.seq_p()))
    rows += [bytes([a]) for a in range(256)] + [bytes([a, b]) for a in range(256) for b in range(256)]
    e16 = uc.corpus_e16()
    rows += [e16.string(i) for i in range(len(e16))]
    cut += [False] * (len(rows) - len(cut))
    lens = np.array([len(r) for r in rows], dtype=np.int64)
    assert lens.max() == 123 and lens.min() == 1
    data = np.zeros((len(rows), 123), dtype=np.uint8)
    for L in np.unique(lens):
        idx = np.nonzero(lens == L)[0]
        data[idx, :L] = np.frombuffer(b"".join(rows[i] for i in idx), dtype=np.uint8).reshape(len(idx), L)
    ok = np.fromiter((uc.valid(r) for r in rows), dtype=bool, count=len(rows))
    return data, lens, ok, np.array(cut)


@pytest.fixture(scope="module")
def reasons():
    return reason_corpus()


def test_the_reason_corpus_holds_both_verdicts_where_it_matters(reasons):
    data, lens, ok, cut = reasons
    for L in (1, 2, 3, 4):
        assert ok[lens == L].any() and (~ok[lens == L]).any(), L
    assert ok[cut].any() and (~ok[cut]).any()         # a whole sequence at the end; one cut by the end
    assert len(lens) > 130000


@FORMS
def test_close_reasons_from_the_conformance_corpus(ctx, cuda, reasons, max_len):
    """A decode's output written by hand, vectorised: per read a PING, the CLOSE
    with the reason, a PING, their payloads packed in ctl with hostile bytes
    around the reason, which starts at ctl offset a mod 4."""
    data, lens, ok, _ = reasons
    n = len(lens)
    host = np.random.default_rng(4)
    for a in range(4):
        p1 = (a + 2) % 4 + 4                          # the first PING's payload: the reason starts at p1 + 2
        assert (p1 + 2) % 4 == a
        ctl = uc.hostile(host, n * SLOT).copy().reshape(n, SLOT)
        ctl[:, p1:p1 + 2] = (0x03, 0xE8)
        cols = np.arange(123)
        mask = cols[None, :] < lens[:, None]
        ctl[:, p1 + 2:p1 + 2 + 123][mask] = data[mask]
        clen = lens + 2
        msgs = np.zeros((n, 3), dtype=_lib.MSG_INFO)
        msgs["n_data_frames"] = 1
        msgs["first_frame"] = msgs["last_frame"] = np.arange(3)[None, :]
        msgs["opcode"] = (PING, CLOSE, PING)
        msgs["off"][:, 1], msgs["off"][:, 2] = p1, p1 + clen
        msgs["len"][:, 0], msgs["len"][:, 1], msgs["len"][:, 2] = p1, clen, 8
        mres = np.zeros(n, dtype=_lib.MSG_RESULT)
        mres["n_msgs"], mres["err_frame"], mres["open_first_frame"] = 3, cc.NONE, cc.NONE
        mres["ctl_bytes"] = p1 + clen + 8
        assert int(mres["ctl_bytes"].max()) <= SLOT
        reads = np.zeros(n, dtype=_lib.MSG_READ)
        reads["ctl_off"] = np.arange(n, dtype=np.uint64) * SLOT
        reads["conn"], reads["dst_cap"], reads["ctl_cap"] = np.arange(n), 16, SLOT
        reads["msg_base"], reads["msg_cap"] = 3 * np.arange(n), 3
        regions = np.zeros(n, dtype=_lib.REPLY_REGION)
        regions["out_off"], regions["out_cap"] = np.arange(n, dtype=np.uint64) * SLOT, SLOT

        def dev(x):
            return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(cuda)

        d = dict(reads=dev(reads), msgs=dev(msgs), ctl=dev(ctl), mres=dev(mres), regions=dev(regions))
        u8 = dict(dtype=torch.uint8, device=cuda)
        dst, flows = torch.zeros(16, **u8), torch.zeros(n * fm.SSZ, **u8)
        out, res = torch.full((n * SLOT,), FILL, **u8), torch.zeros(n * rp.RSZ, **u8)
        tx, st = torch.zeros(n * rp.TSZ, **u8), torch.zeros(n * rp.SSZ, **u8)
        assert gpu.reply_messages_strict(ctx, d["reads"], n, max_len, d["msgs"], dst, d["ctl"], d["mres"], flows, fm.SSZ,
                                         0, d["regions"], out, None, res, tx, st, n, BOTH) == 0
        torch.cuda.synchronize()
        got_res = np.frombuffer(res.cpu().numpy().tobytes(), dtype=_lib.TX_RESULT)
        got_st = np.frombuffer(st.cpu().numpy().tobytes(), dtype=_lib.REPLY_STATE)
        want_len = 2 + p1 + np.where(ok, 2 + clen, 4)
        assert (got_res["status"] == 0).all() and (got_res["n_frames"] == 2).all()
        bad = np.nonzero(got_st["fail_code"] != np.where(ok, 0, 1007))[0]
        assert bad.size == 0, (a, int(bad[0]), data[bad[0], :lens[bad[0]]].tobytes().hex(), int(got_st["fail_code"][bad[0]]))
        assert (got_res["out_len"] == want_len).all()
        assert (got_st["close_sent"] == 1).all() and (got_st["close_code"] == 1000).all()
        assert not flows.any() and torch.equal(d["ctl"], dev(ctl))
        got = out.cpu().numpy().reshape(n, SLOT)
        for i in np.random.default_rng(40 + a).choice(n, 3000, replace=False):
            reason = data[i, :lens[i]].tobytes()
            want = bytes([0x8A, p1]) + ctl[i, :p1].tobytes() + \
                (bytes([0x88, 2 + len(reason), 0x03, 0xE8]) + reason if ok[i] else FAIL[1007])
            assert got[i].tobytes() == want + rp.fill * (SLOT - len(want)), (a, int(i), reason.hex())


# ------------------------------------------------------------------ 5. order
@FORMS
def test_order(ctx, cuda, max_len):
    rng = random.Random(5)
    bad = frame(TEXT, b"caf\xc3", key=key(rng))
    closing = frame(CLOSE, struct.pack(">H", 1000) + b"bye", key=key(rng))
    streams = [[bad + closing], [closing + bad],
               [frame(PING, b"hi", key=key(rng)) + frame(BIN, b"b", key=key(rng)) + bad + frame(PING, b"late", key=key(rng))],
               [frame(PING, b"", key=key(rng)) + frame(BIN, b"an open part", fin=0, key=key(rng)) +
                frame(TEXT, b"not now", key=key(rng))]]
    rc, calls = rounds(ctx, cuda, streams, max_len=max_len)
    wires = [calls[0].region(i) for i in range(4)]
    assert wires[0] == FAIL[1007]
    assert wires[1] == b"\x88\x05\x03\xe8bye"
    assert wires[2] == b"\x8a\x02hi\x82\x01b" + FAIL[1007]
    assert wires[3] == b"\x8a\x00\x02\x0can open part" + FAIL[1002]
    assert fail_codes(rc) == [1007, 0, 1007, 1002]
    assert [r.state["close_code"] for r in rc.ref] == [0, 1000, 0, 0]
    assert [r.tx["last_msg_not_fin"] for r in rc.ref] == [0, 0, 0, 1]


# ------------------------------------------------------------------ 6. the failing frame at every chunk position
@FORMS
def test_the_failing_frame_at_every_chunk_position(ctx, cuda, max_len):
    """Behind a 2-byte PONGs and b 3-byte echoes the failing frame starts at
    2 a + 3 b: every offset from 0 to 17 but 1."""
    rng = random.Random(6)
    reads, offs = [], []
    for o in [0] + list(range(2, 18)):
        b = o % 2
        a = (o - 3 * b) // 2
        assert a >= 0 and 2 * a + 3 * b == o
        w = b"".join(frame(PING, b"", key=key(rng)) for _ in range(a))
        w += b"".join(frame(BIN, bytes([65 + j]), key=key(rng)) for j in range(b))
        reads.append(dict(wire=w + frame(TEXT, b"\xff", key=key(rng)), conn=len(reads)))
        offs.append(o)
    conns, rc = fm.Conns(cuda, len(reads)), SConns(cuda, len(reads))
    _, sp = step(ctx, cuda, conns, rc, reads, max_len)
    for i, o in enumerate(offs):
        assert int(sp.outs[i]["records"][-1]["hdr_off"]) == o and sp.outs[i]["res"]["out_len"] == o + 4
        assert sp.region(i)[o:] == FAIL[1007]
    assert sp.outs[0]["res"]["n_frames"] == 1         # the only frame of its read


@FORMS
def test_the_failing_frame_as_frame_258(ctx, cuda, max_len):
    rng = random.Random(66)
    opener = frame(BIN, cc.payload(rng, 30), key=key(rng))
    ones = [frame(TEXT if j % 3 else BIN, bytes([65 + j % 26]), key=key(rng)) for j in range(256)]
    conns, rc = fm.Conns(cuda, 2), SConns(cuda, 2)
    step(ctx, cuda, conns, rc, [dict(wire=opener[:16], conn=c) for c in range(2)], max_len)
    reads = [dict(wire=opener[16:] + b"".join(ones), conn=c) for c in range(2)]
    # 257 entries and, by hand, a decode error behind them; connection 1 an open part as well: 259 frames
    by_hand = [dict(mres=dict(status=SEQUENCE)), dict(mres=dict(status=SEQUENCE, open_opcode=BIN, open_len=1, open_off=0))]
    outs, sp = step(ctx, cuda, conns, rc, reads, max_len, opts=by_hand)
    assert [len(o["entries"]) for o in outs] == [257, 257]
    assert sp.outs[0]["res"]["n_frames"] == 258 and sp.outs[0]["frames"][-1] == (CLOSE, 1, b"\x03\xea")
    assert sp.region(0)[-4:] == FAIL[1002] and fail_codes(rc) == [1002, 0]
    assert sp.outs[1]["res"] == dict(rr.tr.refusal(INVALID))


# ------------------------------------------------------------------ 7. across reads
def cut_at(wire, *at):
    edges = [0, *at, len(wire)]
    return [wire[a:b] for a, b in zip(edges, edges[1:])]


@FORMS
def test_across_reads(ctx, cuda, max_len):
    L = 30
    hdr = 6                                           # a masked header with a 7-bit length
    broken = cut_at(frame(TEXT, b"ab\xe2\x82\x28cd", key=K), hdr + 3, hdr + 4, hdr + 5)
    mended = cut_at(frame(TEXT, b"ab\xe2\x82\xaccd", key=K), hdr + 3, hdr + 4, hdr + 5)
    exact = cut_at(frame(BIN, bytes(range(L)), key=K), hdr + 10, hdr + 20)
    parts = [frame(BIN, b"0123456789", fin=0, key=K), frame(CONT, b"0123456789", fin=0, key=K)]
    at_limit, over = parts + [frame(CONT, b"0123456789", key=K)], parts + [frame(CONT, b"0123456789X", key=K)]
    announced = cut_at(frame(BIN, bytes(L + 1), key=K), hdr + 1)
    rc, calls = rounds(ctx, cuda, [broken, mended, exact, at_limit, over, announced], limit=L, max_len=max_len)
    per_read = [int(sp.outs[0]["res"]["out_len"]) for sp in calls]   # (connection 0 is read 0 of every round)
    assert fail_codes(rc) == [1007, 0, 0, 0, 1009, 1009]
    # the broken sequence fails in the read that brings 28, the third, and the fourth is met with silence
    assert rc.ref[0].wire == b"\x01\x03ab\xe2\x00\x01\x82" + FAIL[1007] and per_read == [5, 3, 4, 0]
    assert rr.messages(rr.walk_frames(rc.ref[1].wire))[0] == [(TEXT, b"ab\xe2\x82\xaccd")]
    assert rr.messages(rr.walk_frames(rc.ref[2].wire))[0] == [(BIN, bytes(range(L)))]
    assert rr.messages(rr.walk_frames(rc.ref[3].wire))[0] == [(BIN, b"0123456789" * 3)]
    assert rc.ref[4].wire == b"\x02\x0a0123456789\x00\x0a0123456789" + FAIL[1009]
    assert rc.ref[5].wire == FAIL[1009]               # in the read that holds the header


def test_stride_64_after_decode_messages_multi(ctx, cuda):
    """Whole-frame reads through fws_gpu_decode_messages_multi, the strict reply over its carries."""
    L = 30
    parts = [frame(BIN, b"0123456789", fin=0, key=K), frame(CONT, b"0123456789", fin=0, key=K)]
    streams = [parts + [frame(CONT, b"0123456789", key=K)], parts + [frame(CONT, b"0123456789X", key=K)],
               [frame(TEXT, b"ab\xe2", fin=0, key=K), frame(CONT, b"\x82", fin=0, key=K), frame(CONT, b"\x28", fin=0, key=K)],
               [frame(TEXT, b"ab\xe2", fin=0, key=K), frame(CONT, b"\x82", fin=0, key=K), frame(CONT, b"\xac", key=K)],
               [frame(PING, b"p", key=K) + frame(CONT, b"x", key=K)], [frame(CLOSE, b"\x03\xe8\xc3", key=K)]]
    n = len(streams)
    conns, rc = mm.Conns(cuda, n), SConns(cuda, n, BOTH, L)
    for k in range(3):
        live = [c for c in range(n) if k < len(streams[c])]
        _, m, _ = mm.run(ctx, cuda, conns, [dict(wire=streams[c][k], conn=c) for c in live])
        strict(ctx, cuda, m, rc)
    assert fail_codes(rc) == [0, 1009, 1007, 0, 1002, 1007]
    assert rc.ref[1].wire.endswith(b"\x00\x0a0123456789" + FAIL[1009])
    assert rc.ref[2].wire == b"\x01\x03ab\xe2\x00\x01\x82" + FAIL[1007]
    assert rc.ref[4].wire == b"\x8a\x01p" + FAIL[1002] and rc.ref[5].wire == FAIL[1007]


# ------------------------------------------------------------------ 8. after the failure
def test_after_the_failure(ctx, cuda):
    rng = random.Random(8)
    bad = frame(BIN, b"ok", key=key(rng)) + frame(TEXT, b"\xc0\xaf", key=key(rng))
    good = frame(BIN, b"neighbour", key=key(rng)) + frame(PING, b"n", key=key(rng))
    conns, rc = fm.Conns(cuda, 3), SConns(cuda, 3)
    rc.preset(2, close_sent=1)                        # the host closed connection 2 itself
    rc.check()
    _, sp = step(ctx, cuda, conns, rc, [dict(wire=bad, conn=0), dict(wire=good, conn=1), dict(wire=bad, conn=2)])
    assert sp.region(0) == b"\x82\x02ok" + FAIL[1007] and sp.outs[1]["res"]["n_frames"] == 2
    assert sp.outs[2]["res"] == dict(rr.tr.refusal(0))
    assert fail_codes(rc) == [1007, 0, 0]
    states = rc.st.clone()
    _, sp = step(ctx, cuda, conns, rc, [dict(wire=good, conn=c) for c in range(3)])
    assert [o["res"]["n_frames"] for o in sp.outs] == [0, 2, 0] and torch.equal(states, rc.st)
    assert rc.ref[0].state == dict(close_sent=1, close_code=0, fail_code=1007, reserved=0)
    assert rc.ref[0].tx["frames"] == 2 and rc.ref[2].tx["frames"] == 0


# ------------------------------------------------------------------ 9. capacity
def test_capacity_counts_the_failing_frame(ctx, cuda):
    rng = random.Random(9)
    wire = rp.binmsg(rng, 200) + frame(PING, b"ping", key=key(rng)) + frame(TEXT, b"\xf5", key=key(rng)) + rp.binmsg(rng, 50)
    need = 204 + 6 + 4
    conns, rc = fm.Conns(cuda, 2), SConns(cuda, 2)
    _, m, _ = fm.run(ctx, cuda, conns, [dict(wire=wire, conn=0), dict(wire=wire, conn=1)])
    sp = strict(ctx, cuda, m, rc, opts=[dict(out_cap=need - 1), dict(out_cap=need)])
    assert sp.outs[0]["res"] == rr.tr.refusal(CAPACITY, 3, need) and sp.outs[1]["res"]["out_len"] == need
    assert rc.ref[0].tx == rr.new_tx() and rc.ref[0].state == fail_ref.new_state() and fail_codes(rc) == [0, 1007]
    m.outs[1] = rr.undecoded(_lib.FWS_ERR_DECLINED)   # (connection 1 is done: its read is not answered twice)
    sp = Strict(cuda, m, rc, opts=[dict(out_cap=need), dict(out_cap=need, mres=dict(status=_lib.FWS_ERR_DECLINED))])
    sp.expect()
    sp.launch(ctx)
    torch.cuda.synchronize()
    sp.check()
    rc.check()
    assert sp.outs[0]["res"]["status"] == 0 and sp.region(0) == rc.ref[1].wire and fail_codes(rc) == [1007, 1007]


# ------------------------------------------------------------------ 10. queued on one stream
def test_three_rounds_queued_on_one_stream(ctx, cuda):
    n, failing = 8, 3
    rng = random.Random(10)
    conns, rc = fm.Conns(cuda, n), SConns(cuda, n)
    calls = []
    for k in range(3):
        reads = []
        for c in range(n):
            text = b"\xe2\x28\xa1" if (k == 1 and c == failing) else cc.random_text(rng, 40 + c)
            reads.append(dict(wire=rp.binmsg(rng, 10 + 7 * c) + frame(PING, bytes([48 + k]), key=key(rng)) +
                              frame(TEXT, text, key=key(rng)), conn=c))
        m = fm.Flow(cuda, conns, reads)
        m.expect()
        sp = Strict(cuda, m, rc)
        sp.expect()
        calls.append((m, sp))
    torch.cuda.synchronize()
    for m, sp in calls:                               # six launches, nothing in between
        m.launch(ctx)
        sp.launch(ctx)
    torch.cuda.synchronize()
    for m, sp in calls:
        m.check()
        sp.check()
    conns.check()
    rc.check()
    assert fail_codes(rc) == [1007 if c == failing else 0 for c in range(n)]
    assert [sp.outs[failing]["res"]["n_frames"] for _, sp in calls] == [3, 3, 0]
    assert all(o["res"]["n_frames"] == 3 for _, sp in calls for c, o in enumerate(sp.outs) if c != failing)


# ------------------------------------------------------------------ 11. MessageResponder(strict=True)
def test_message_responder_strict(ctx, cuda):
    groups = {}
    for case in CASES:
        groups.setdefault((case[2], case[3]), []).append(case)
    for (flags, limit), cases in groups.items():
        for is_strict in (True, False):
            flow = gpu.MessageFlow(ctx, len(cases), max_read=1024)
            responder = gpu.MessageResponder(flow, flags, strict=is_strict, max_message=limit)
            assert responder.out_slot >= flow.slot + 10 * (flow.msg_cap + 1) + (4 if is_strict else 0)
            replies = [b""] * len(cases)
            for k in range(max(len(c[1]) for c in cases)):
                feed = {i: c[1][k] for i, c in enumerate(cases) if k < len(c[1]) and
                        flow.status[i] in (0, CAPACITY)}
                if not feed:
                    continue
                _, back = responder.feed(feed)
                for i, b in back.items():
                    replies[i] += b
            for i, (name, reads, _, _, want, code) in enumerate(cases):
                if is_strict:
                    assert replies[i] == bytes.fromhex(want), name
                    assert responder.failed.get(i, 0) == code, name
                else:                                 # as before: the plain call's answer
                    ref, pending, f = rr.ReplyRef(flags), b"", fm.FlowRef()
                    for data in reads:
                        out = f.call(pending + data)
                        pending = (pending + data)[out["res"]["resume_off"]:]
                        ref.call(out)
                        if out["res"]["status"] not in (0, CAPACITY):
                            break
                    assert replies[i] == ref.wire, name
            assert (set(responder.failed) == {i for i, c in enumerate(cases) if c[5]}) if is_strict else \
                not responder.failed
