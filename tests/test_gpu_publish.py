"""GPU parity of fws_gpu_publish_messages: messages fanned out to many
connections in one launch.

The oracle is publish_ref.predict (test_publish_cpu.py holds it against
txmulti_ref and through it against the reference's recorded frames). Everything
a call writes lies in one arena pre-filled with a sentinel: every subscriber's
region with a guard in front of and behind it, the result array, every slice of
frame records and a guard record behind it; the arena is compared whole with the
model's. The connections' two state arrays hold connection c at index 2c, the odd
records are guards, and are compared whole as well. What a call only reads -- the
records, the lists, the subscribers, the three source buffers -- lies in a second
arena that must come back unchanged. All comparisons are exact."""
import hashlib
import random

import numpy as np
import pytest
import torch

import publish_ref as pr
import reply_ref as rr
import test_gpu_join as gj
import test_gpu_msg_flow as fm
import txmulti_ref as tr
from flashws_amd import _lib, gpu

pytestmark = pytest.mark.gpu

FILL, GUARD = 0xA5, 64
SMALL, FULL = 16 << 10, _lib.FWS_TX_MULTI_MAX_SEND
FORMS = pytest.mark.parametrize("max_len", [SMALL, FULL], ids=["small", "full"])
TSZ, SSZ, RSZ, FSZ, PSZ, JSZ = (_lib.TX_CONN.itemsize, _lib.REPLY_STATE.itemsize, _lib.TX_RESULT.itemsize,
                                _lib.FRAME_INFO.itemsize, _lib.PUB_SUB.itemsize, _lib.JOIN_INFO.itemsize)
TEXT, BIN, CLOSE, PING, PONG = 1, 2, 8, 9, 10
IN_DST, IN_STORE, IN_CTL, NOWHERE = pr.IN_DST, pr.IN_STORE, pr.IN_CTL, pr.NOWHERE
FRAME_GUARD = 3                                           # guard records behind a slice of frame records


def align(v, a):
    return (v + a - 1) // a * a


class PConns:
    """The send side of a test's connections: fws_tx_conn and fws_reply_state
    arrays on the device -- record 2c is connection c's, the odd records are
    guards -- and the model's states."""

    def __init__(self, cuda, n):
        self.n, self.n_dev, self.cuda = n, 2 * n, cuda
        self.tx, self.st = [pr.new_tx() for _ in range(n)], [pr.new_state() for _ in range(n)]
        self.conns, self.states = self._array(TSZ), self._array(SSZ)

    def _array(self, sz):
        host = np.full(self.n_dev * sz + GUARD, FILL, dtype=np.uint8)
        for c in range(self.n):
            host[2 * c * sz:(2 * c + 1) * sz] = 0
        return torch.from_numpy(host).to(self.cuda)

    def preset(self, c, tx=None, st=None):
        """States written by hand: what an earlier call, or the host, left."""
        if tx:
            self.tx[c] = dict(self.tx[c], **tx)
            rec = np.frombuffer(pr.tx_bytes(self.tx[c]), dtype=np.uint8).copy()
            self.conns[2 * c * TSZ:(2 * c + 1) * TSZ] = torch.from_numpy(rec).to(self.cuda)
        if st:
            self.st[c] = dict(self.st[c], **st)
            rec = np.frombuffer(pr.state_bytes(self.st[c]), dtype=np.uint8).copy()
            self.states[2 * c * SSZ:(2 * c + 1) * SSZ] = torch.from_numpy(rec).to(self.cuda)

    def check(self):
        for t, sz, ref, to_bytes in ((self.conns, TSZ, self.tx, pr.tx_bytes), (self.states, SSZ, self.st, pr.state_bytes)):
            raw = t.cpu().numpy().tobytes()
            want = b"".join(to_bytes(ref[c]) + bytes([FILL]) * sz for c in range(self.n)) + bytes([FILL]) * GUARD
            if raw != want:
                at = next(i for i in range(len(raw)) if raw[i] != want[i])
                assert False, ("state array", sz, "record", at // sz, "differs at byte", at % sz)


class Pub:
    """One publish call. recs: JOIN_INFO records; bufs: the bytes of (dst, store,
    ctl), None for a base passed as NULL; subs: dicts -- conn, lst (a Python
    list of indices; the same list object is laid out once and shared), and
    optionally out_cap, frame_cap, desc (fws_pub_sub fields overridden last) and
    list_ok / conn_ok (what the model is told about an overridden field).
    mis[w]: base w starts this many bytes past a 256-B boundary."""

    def __init__(self, cuda, pc, recs, bufs, subs, max_len, mis=(0, 0, 0), n_msgs=None, n_list=None):
        self.cuda, self.pc, self.recs, self.subs, self.max_len, self.n = cuda, pc, recs, subs, max_len, len(subs)
        self.bufs = [None if b is None else np.frombuffer(bytes(b), dtype=np.uint8) for b in bufs]
        self.n_msgs = len(recs) if n_msgs is None else n_msgs
        # ---- what the call reads
        off, self.inp = 0, {}
        lists, flat = {}, []
        for s in subs:
            if id(s["lst"]) not in lists:
                lists[id(s["lst"])] = len(flat)
                flat += s["lst"]
            s["list_off"] = lists[id(s["lst"])]
        self.n_lists = len(lists)
        self.n_list = len(flat) if n_list is None else n_list
        parts = [("recs", recs.view(np.uint8).reshape(-1), 0), ("list", np.asarray(flat, dtype=np.uint32).view(np.uint8), 0)]
        parts += [(f"base{w}", b, mis[w]) for w, b in enumerate(self.bufs) if b is not None]
        for k, data, m in parts:
            o = align(off + GUARD, 256) + m
            self.inp[k] = (o, len(data))
            off = o + max(len(data), 16)
        o = align(off + GUARD, 256)
        self.inp["subs"] = (o, self.n * PSZ)
        off = o + self.n * PSZ
        # ---- what the call writes
        out, fb = 0, 0
        for s in subs:
            s.setdefault("out_cap", sum(int(recs[i]["len"]) + 10 for i in s["lst"]
                                        if i < len(recs) and not pr.is_nothing(recs[i])) + 16)
            s.setdefault("frame_cap", len(s["lst"]))
            s["out_off"] = align(out + GUARD, 256)
            out = s["out_off"] + s["out_cap"]
            s["fb"] = fb
            fb += s["frame_cap"] + FRAME_GUARD
        self.sec = {}
        for k, sz in (("frames", fb * FSZ), ("res", self.n * RSZ)):
            o = align(out + GUARD, 256)
            self.sec[k] = (o, sz)
            out = o + sz
        host_in = np.full(align(off + GUARD, 256), FILL, dtype=np.uint8)
        for k, data, _ in parts:
            host_in[self.inp[k][0]:self.inp[k][0] + len(data)] = data
        desc = np.zeros(self.n, dtype=_lib.PUB_SUB)
        for i, s in enumerate(subs):
            desc[i] = (s["out_off"], s["out_cap"], 2 * s["conn"], s["list_off"], len(s["lst"]), s["fb"], s["frame_cap"])
            for k, v in s.get("desc", {}).items():
                desc[i][k] = v
        self.desc = desc
        host_in[self.inp["subs"][0]:][:self.n * PSZ] = desc.view(np.uint8)
        self.host_in = host_in
        self.inputs = torch.from_numpy(host_in).to(cuda)
        self.host_out = np.full(align(out + GUARD, 256), FILL, dtype=np.uint8)
        self.arena = torch.from_numpy(self.host_out).to(cuda)
        assert self.inputs.data_ptr() % 256 == 0 and self.arena.data_ptr() % 256 == 0

    def i(self, k):
        if k not in self.inp:
            return None
        o, sz = self.inp[k]
        return self.inputs[o:o + max(sz, 16)]

    def src_addr(self, rec):
        """A record's source address mod 16."""
        return (self.inp[f"base{int(rec['where'])}"][0] + int(rec["off"])) & 15

    def expect(self, cache=None):
        """The model advanced by this call; the arena as it must look afterwards."""
        want = self.host_out.copy()
        self.outs = []
        for i, s in enumerate(self.subs):
            c = s["conn"]
            d = self.desc[i]
            got = pr.predict(self.pc.tx[c], self.pc.st[c], self.recs[:self.n_msgs], self.bufs, s["lst"],
                             max_len=self.max_len, out_cap=int(d["out_cap"]), frame_cap=int(d["frame_cap"]),
                             out_off=int(d["out_off"]), conn_ok=s.get("conn_ok", True),
                             list_ok=s.get("list_ok", True), cache=cache)
            self.pc.tx[c], self.pc.st[c] = got["tx"], got["state"]
            self.outs.append(got)
            o = s["out_off"]
            want[o:o + len(got["bytes"])] = np.frombuffer(got["bytes"], dtype=np.uint8)
            o = self.sec["frames"][0] + s["fb"] * FSZ
            rec = got["records"].tobytes()
            want[o:o + len(rec)] = np.frombuffer(rec, dtype=np.uint8)
            r = np.zeros(1, dtype=_lib.TX_RESULT)
            for k, v in got["res"].items():
                r[0][k] = v
            o = self.sec["res"][0] + i * RSZ
            want[o:o + RSZ] = r.view(np.uint8)
        self.want = want
        return self.outs

    def launch(self, ctx, stream=None, frames=True):
        o, sz = self.sec["frames"]
        rc = gpu.publish_messages(ctx, self.i("recs"), self.n_msgs, self.i("base0"), self.i("base1"), self.i("base2"),
                                  self.i("list"), self.n_list, self.i("subs"), self.n, self.max_len, self.arena,
                                  self.arena[o:] if frames else None, self.arena[self.sec["res"][0]:],
                                  self.pc.conns, self.pc.states, self.pc.n_dev, stream=stream)
        assert rc == 0, rc

    def check(self):
        got = self.got = self.arena.cpu().numpy()
        res = np.frombuffer(got[self.sec["res"][0]:][:self.n * RSZ].tobytes(), dtype=_lib.TX_RESULT)
        for i, out in enumerate(self.outs):
            for k in _lib.TX_RESULT.names:
                assert int(res[i][k]) == out["res"][k], ("result", i, k, int(res[i][k]), out["res"][k])
        if not np.array_equal(got, self.want):
            at = int(np.nonzero(got != self.want)[0][0])
            s = max((s for s in self.subs if s["out_off"] <= at), key=lambda s: s["out_off"], default=None)
            assert False, ("the arena differs at", at, "subscriber", self.subs.index(s) if s else None, "offset",
                           at - s["out_off"] if s else None, int(got[at]), int(self.want[at]), self.sec)
        assert np.array_equal(self.inputs.cpu().numpy(), self.host_in), "the call's inputs were modified"


def run(ctx, cuda, pc, recs, bufs, subs, max_len, cache=None, **kw):
    """One call, checked in full."""
    p = Pub(cuda, pc, recs, bufs, subs, max_len, **kw)
    outs = p.expect(cache)
    p.launch(ctx)
    torch.cuda.synchronize()
    p.check()
    pc.check()
    return outs, p


def sources(seed, size):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size, dtype=np.uint8).tobytes() for _ in range(3)]


def statuses(outs):
    return [o["res"]["status"] for o in outs]


# ------------------------------------------------------------------ 1. seams
SEAM_LENS = (0, 1, 2, 3, 13, 14, 15, 16, 17, 125, 126)
SEAM_BIG = (65535, 65536)


@FORMS
def test_seam_lengths_at_every_source_misalignment(ctx, cuda, max_len):
    """Frames of 0, 1, 2, 3 (six in one chunk), 13 .. 17 bytes and both sides of
    the header classes, each at source misalignments 0 .. 15, the three bases
    mixed in one region."""
    lens = SEAM_LENS + (SEAM_BIG if max_len == FULL else ())
    bufs = sources(1, 16 * (70 << 10) if max_len == FULL else 16 * 1024)
    items, at = [], [0, 0, 0]
    for m in range(16):
        for j, ln in enumerate(lens):
            w = (m + j) % 3
            off = align(at[w], 16) + m
            at[w] = off + ln
            items.append((BIN if (m + j) & 1 else TEXT, w, off, ln) if ln > 125 or j % 4 else (PING, w, off, ln))
    recs = pr.records(items)
    L = len(lens)
    subs, conn = [], 0
    for m in range(16):
        mine = list(range(m * L, (m + 1) * L))
        for lst in (mine, mine[::-1], [(i * L + (i + m) % L) for i in range(16)],
                    [m * L + k for k in (0, 0, 1, 0, 1, 2, 3, 3, 2, 1)]):
            subs.append(dict(conn=conn, lst=lst))
            conn += 1
    pc = PConns(cuda, conn)
    outs, p = run(ctx, cuda, pc, recs, bufs, subs, max_len, mis=(0, 5, 11))
    assert statuses(outs) == [0] * len(subs)
    assert {p.src_addr(r) for r in recs} == set(range(16))
    # six frames in one 16-B chunk: the frames of 0 .. 3 bytes are 2 .. 5 bytes each
    short = outs[3]["records"]
    assert [int(r["hdr_off"]) for r in short[:7]] == [0, 2, 4, 7, 9, 12, 16] and len(short) == 10


def seam_class_subs(max_len):
    """A deterministic sweep: per header class H and per total mod 16, two lists
    of a lead frame and 128 frames of the class whose sizes advance the payload
    start by 1 mod 16 per frame and by 2 on every 16th, while the source
    misalignment advances by 1: every (payload start, source address) pair mod
    16. The lead frame's length sets the total mod 16."""
    classes = [(2, 0), (4, 126)] + ([(10, 65536)] if max_len == FULL else [])
    items, index, subs, at = [], {}, [], [0, 0, 0]

    def rec(op, w, mis, ln):
        key = (op, w, mis, ln)
        if key not in index:                              # one record per distinct frame: the lists share them
            off = align(at[w], 16) + mis
            at[w] = off + ln
            index[key] = len(items)
            items.append((op, w, off, ln))
        return index[key]

    for H, base in classes:
        for t in range(16):
            for half in range(2):
                lst = [rec(PING, t % 3, t, t)]            # the lead: 2 + t bytes
                for k in range(128 * half, 128 * half + 128):
                    step = 2 if k % 16 == 15 else 1
                    ln = base + (step - H - base) % 16
                    # (the second half's sources stand 8 further: the other eight diagonals)
                    lst.append(rec(BIN if k & 1 else TEXT, k % 3, (k + 8 * half) % 16, ln))
                subs.append(dict(conn=len(subs), lst=lst))
    return items, subs, at


@FORMS
def test_every_seam_class_is_reached(ctx, cuda, max_len):
    """Every (header size, payload start mod 16, source address mod 16, total mod
    16) class, counted from the model's frame records and the records' device
    addresses."""
    items, subs, at = seam_class_subs(max_len)
    bufs = sources(2, max(at) + 16)
    recs = pr.records(items)
    pc = PConns(cuda, len(subs))
    outs, p = run(ctx, cuda, pc, recs, bufs, subs, max_len, cache={}, mis=(0, 0, 0))
    assert statuses(outs) == [0] * len(subs)
    seen = set()
    for s, out in zip(subs, outs):
        total = out["res"]["out_len"]
        assert len(out["records"]) == len(s["lst"])
        for i, fr in zip(s["lst"], out["records"]):
            seen.add((int(fr["hdr_len"]), (int(fr["hdr_off"]) + int(fr["hdr_len"])) & 15, p.src_addr(recs[i]), total & 15))
    hs = (2, 4, 10) if max_len == FULL else (2, 4)
    missing = [(h, a, b, t) for h in hs for a in range(16) for b in range(16) for t in range(16)
               if (h, a, b, t) not in seen]
    assert not missing, (len(missing), missing[:8])
    assert {out["res"]["out_len"] & 15 for out in outs} == set(range(16))


# ------------------------------------------------------------------ 2. lists
@FORMS
def test_list_lengths_and_a_list_shared_by_64(ctx, cuda, max_len):
    rng = random.Random(3)
    bufs = sources(3, 8192)
    lens = [rng.choice([0, 1, 5, 16, 40, 125, 126, 300]) for _ in range(40)]
    items = [(rng.choice([TEXT, BIN]) if ln > 125 or i % 5 else rng.choice([PING, PONG]), i % 3,
              rng.randrange(0, 7000), ln) for i, ln in enumerate(lens)]
    items += [(0, 0, 0, 0), (BIN, NOWHERE, 0, 50), (0, NOWHERE, 0, 1 << 40), (0, 200, 1 << 50, 7)]   # 40 .. 43: nothing
    recs = pr.records(items)
    room = [rng.randrange(40) for _ in range(30)]
    need = sum(tr.hdr_len(lens[i], False) + lens[i] for i in room)
    subs = [dict(conn=c, lst=room, out_cap=need + (c % 7) - 3) for c in range(64)]       # some too small
    c = 64
    for lst in ([], [7], [i % 40 for i in range(255)], [(3 * i) % 40 for i in range(256)], [i % 40 for i in range(257)],
                [40, 41, 5, 6], [5, 42, 43, 6], [5, 6, 40, 41], [40, 41, 42, 43] * 8, [9, 9], [41] + [12] * 5 + [40]):
        subs.append(dict(conn=c, lst=lst))
        c += 1
    pc = PConns(cuda, c)
    outs, p = run(ctx, cuda, pc, recs, bufs, subs, max_len, mis=(3, 0, 9))
    assert p.n_lists == 12                                # the room's list is in the call once
    assert statuses(outs[:64]) == [0 if (i % 7) - 3 >= 0 else pr.CAPACITY for i in range(64)]
    assert all(o["res"]["out_len"] == need and o["res"]["n_frames"] == 30 for o in outs[:64])
    assert statuses(outs[64:]) == [0, 0, 0, 0, pr.INVALID, 0, 0, 0, 0, 0, 0]
    assert [o["res"]["n_frames"] for o in outs[64:]] == [0, 1, 255, 256, 0, 2, 2, 2, 0, 2, 5]
    assert outs[73]["bytes"][:len(outs[73]["bytes"]) // 2] == outs[73]["bytes"][len(outs[73]["bytes"]) // 2:]


@FORMS
def test_256_items_one_per_thread(ctx, cuda, max_len):
    """256 frames of unequal sizes: in the 256-thread form every thread has an
    item and every wave's scan carry is used; in the 1024-thread form three
    quarters of the threads have none."""
    rng = random.Random(4)
    top = 3000 if max_len == SMALL else 20000
    bufs = sources(4, 256 * 64 + top + 4096)
    items = []
    for i in range(256):
        ln = rng.choice([0, 1, 2, 15, 16, 17, 100, 125, 126, 127, rng.randrange(top)])
        items.append((rng.choice([TEXT, BIN]) if ln > 125 or i % 3 else PING, i % 3, rng.randrange(0, 256 * 64), ln))
    recs = pr.records(items)
    order = list(range(256))
    rng.shuffle(order)
    subs = [dict(conn=0, lst=list(range(256))), dict(conn=1, lst=order), dict(conn=2, lst=order, frame_cap=100)]
    pc = PConns(cuda, 3)
    outs, p = run(ctx, cuda, pc, recs, bufs, subs, max_len, mis=(1, 2, 3))
    assert [o["res"]["n_frames"] for o in outs] == [256] * 3 and len(outs[2]["records"]) == 100
    assert pc.tx[1]["frames"] == 256 and pc.tx[1]["wire_bytes"] == outs[1]["res"]["out_len"]


# ------------------------------------------------------------------ 3. CLOSE
def test_close_first_in_the_middle_and_last(ctx, cuda):
    bufs = sources(5, 4096)
    bufs[2] = bytes([0x03, 0xE9]) + b"going away" + bufs[2][12:]
    # 0 CLOSE 1001 + reason, 1 TEXT, 2 BIN, 3 PING, 4 over-long PING, 5 empty CLOSE, 6 a data record over max_len
    recs = pr.records([(CLOSE, IN_CTL, 0, 12), (TEXT, IN_DST, 3, 70), (BIN, IN_STORE, 9, 200), (PING, IN_CTL, 40, 8),
                       (PING, IN_CTL, 60, 126), (CLOSE, IN_DST, 0, 0), (BIN, IN_DST, 0, 2000)])
    lists = [[0, 1, 2], [1, 0, 2, 3], [1, 2, 3, 0], [1, 0, 4], [0, 6], [5], [1, 0, 2, 5, 1], [1, 2], [1, 2]]
    subs = [dict(conn=c, lst=lst) for c, lst in enumerate(lists)]
    pc = PConns(cuda, len(subs))
    pc.preset(7, st=dict(close_sent=1, close_code=1000))      # close_sent found set
    pc.preset(6, st=dict(close_code=1002, fail_code=1002))    # left as they were
    outs, p = run(ctx, cuda, pc, recs, bufs, subs, 1024)
    assert statuses(outs) == [0, 0, 0, pr.CONTROL, pr.DECLINED, 0, 0, 0, 0]
    assert [o["res"]["n_frames"] for o in outs] == [1, 2, 4, 0, 0, 1, 2, 0, 2]
    assert [s["close_sent"] for s in pc.st] == [1, 1, 1, 0, 0, 1, 1, 1, 0]
    assert pc.st[6] == dict(close_sent=1, close_code=1002, fail_code=1002, reserved=0)
    assert rr.walk_frames(outs[1]["bytes"]) == [(TEXT, 1, bufs[0][3:73]), (CLOSE, 1, bufs[2][:12])]
    # a second call after the CLOSE, queued behind the first on the same stream, writes nothing
    pc2 = PConns(cuda, 3)
    first = Pub(cuda, pc2, recs, bufs, [dict(conn=0, lst=[1, 0]), dict(conn=1, lst=[1]), dict(conn=2, lst=[3, 5])], 1024)
    second = Pub(cuda, pc2, recs, bufs, [dict(conn=0, lst=[1, 2]), dict(conn=1, lst=[1, 2]), dict(conn=2, lst=[3])], 1024)
    first.expect()
    outs2 = second.expect()
    torch.cuda.synchronize()
    first.launch(ctx)
    second.launch(ctx)
    torch.cuda.synchronize()
    first.check()
    second.check()
    pc2.check()
    assert [o["res"]["n_frames"] for o in outs2] == [0, 2, 0] and statuses(outs2) == [0, 0, 0]
    assert pc2.tx[0]["frames"] == 2 and pc2.tx[1]["frames"] == 3 and pc2.tx[2]["frames"] == 2


# ------------------------------------------------------------------ 4. sequencing
def test_an_open_message_is_not_cut_into(ctx, cuda):
    bufs = sources(6, 4096)
    recs = pr.records([(TEXT, IN_DST, 1, 90), (PING, IN_CTL, 2, 9), (CLOSE, IN_CTL, 20, 2), (PONG, IN_STORE, 7, 0)])
    lists = [[0], [1, 0], [1, 3, 1], [1, 2, 0], [2, 0, 0], [0, 2], [0]]
    subs = [dict(conn=c, lst=lst) for c, lst in enumerate(lists)]
    pc = PConns(cuda, len(subs))
    for c in range(6):
        pc.preset(c, tx=dict(last_msg_not_fin=1, frames=10 + c, wire_bytes=1000))
    pc.preset(4, tx=dict(last_msg_not_fin=7))                 # any non-zero value is an open message; it is kept
    outs, p = run(ctx, cuda, pc, recs, bufs, subs, 512)
    assert statuses(outs) == [pr.SEQUENCE, pr.SEQUENCE, 0, 0, 0, pr.SEQUENCE, 0]
    assert [o["res"]["n_frames"] for o in outs] == [0, 0, 3, 2, 1, 0, 1]
    assert [o["res"]["last_msg_not_fin"] for o in outs] == [0, 0, 1, 1, 1, 0, 0]
    assert [t["last_msg_not_fin"] for t in pc.tx] == [1, 1, 1, 1, 7, 1, 0]
    assert [t["frames"] for t in pc.tx] == [10, 11, 15, 15, 15, 15, 1]


def test_chained_with_the_encode_call_through_one_dev_conns(ctx, cuda):
    """encode (a first fragment, the message left open) -> publish (data refused,
    a PING written) -> encode (the last fragment) -> publish (data written),
    queued on one stream with nothing in between, one fws_tx_conn array."""
    bufs = sources(7, 4096)
    recs = pr.records([(BIN, IN_DST, 5, 300), (PING, IN_CTL, 0, 4)])
    n = 2
    pc = PConns(cuda, n)
    payload = np.frombuffer(sources(8, 1024)[0], dtype=np.uint8)
    src = torch.from_numpy(payload.copy()).to(cuda)
    enc_out = torch.full((2 * n * 2048,), FILL, dtype=torch.uint8, device=cuda)
    enc_res = torch.zeros(2 * n * RSZ, dtype=torch.uint8, device=cuda)
    sends, enc_want = [], []
    for k, (off, ln, last) in enumerate(((0, 500, 0), (500, 524, 1))):
        d = np.zeros(n, dtype=_lib.TX_SEND)
        for c in range(n):
            d[c]["src_off"], d[c]["out_off"], d[c]["len"], d[c]["out_cap"] = off, (k * n + c) * 2048, ln, 2048
            d[c]["conn"], d[c]["frame_type"], d[c]["last"] = 2 * c, TEXT, last
        sends.append(torch.from_numpy(d.view(np.uint8).copy()).to(cuda))
    pubs = [Pub(cuda, pc, recs, bufs, [dict(conn=0, lst=[0, 1]), dict(conn=1, lst=[1, 1])], 512),
            Pub(cuda, pc, recs, bufs, [dict(conn=0, lst=[1, 0]), dict(conn=1, lst=[0])], 512)]
    for k, (off, ln, last) in enumerate(((0, 500, 0), (500, 524, 1))):     # the model, in the stream's order
        for c in range(n):
            got = tr.predict(pc.tx[c], payload[off:off + ln].tobytes(), TEXT, last, masked=False)
            pc.tx[c] = got["state"]
            enc_want.append(got)
        pubs[k].expect()
    torch.cuda.synchronize()
    for k in range(2):
        rc = gpu.encode_messages_multi(ctx, enc_out, src, sends[k], n, 1024, None, enc_res[k * n * RSZ:], pc.conns,
                                       pc.n_dev)
        assert rc == 0
        pubs[k].launch(ctx)
    torch.cuda.synchronize()
    for p in pubs:
        p.check()
    pc.check()
    assert statuses(pubs[0].outs) == [pr.SEQUENCE, 0] and statuses(pubs[1].outs) == [0, 0]
    assert pubs[0].outs[1]["res"]["last_msg_not_fin"] == 1 and pubs[1].outs[0]["res"]["last_msg_not_fin"] == 0
    res = np.frombuffer(enc_res.cpu().numpy().tobytes(), dtype=_lib.TX_RESULT)
    out = enc_out.cpu().numpy()
    for j, got in enumerate(enc_want):
        assert int(res[j]["status"]) == 0 and int(res[j]["out_len"]) == len(got["bytes"])
        assert out[j * 2048:j * 2048 + len(got["bytes"])].tobytes() == got["bytes"]
    # what connection 1 was sent, in order: a first fragment, two PINGs in the middle of the message, its end, a message
    wire = enc_want[1]["bytes"] + pubs[0].outs[1]["bytes"] + enc_want[3]["bytes"] + pubs[1].outs[1]["bytes"]
    units, open_ = rr.messages(rr.walk_frames(wire))
    assert open_ is None and [u[0] for u in units] == [PING, PING, TEXT, BIN] and units[2][1] == payload.tobytes()
    assert pc.tx[1]["frames"] == 5 and pc.tx[0]["frames"] == 4


# ------------------------------------------------------------------ 5. refusals
def test_every_refusal_row_and_the_order_between_rows(ctx, cuda):
    """Every row of the header's table, and for every adjacent pair of rows a
    subscriber that has both causes (the earlier row wins). Good subscribers
    stand between the refused ones and are written as if alone."""
    bufs = sources(9, 140 << 10)
    big = SMALL + 1
    # 0 data, 1 PING, 2 over-long PING, 3 data over max_len, 4 CLOSE, 5 bad opcode, 6 nothing, 7 where above 3,
    # 8 data over FWS_TX_MULTI_MAX_SEND, 9 names the store
    recs = pr.records([(BIN, IN_DST, 3, 100), (PING, IN_CTL, 0, 5), (PING, IN_CTL, 0, 126), (TEXT, IN_DST, 0, big),
                       (CLOSE, IN_CTL, 8, 2), (3, IN_DST, 0, 1), (0, 9, 0, 0), (BIN, 4, 0, 1),
                       (BIN, IN_DST, 0, FULL + 1), (BIN, IN_STORE, 0, 10)])
    good = [0, 1]
    cases = [
        (dict(lst=[0], desc=dict(out_off=8)), pr.INVALID),                     # row 1, cause by cause
        (dict(lst=[0], desc=dict(conn=1000), conn_ok=False), pr.INVALID),
        (dict(lst=[0], desc=dict(list_len=257)), pr.INVALID),
        (dict(lst=[0], desc=dict(list_off=0xFFFFFFFF, list_len=2), list_ok=False), pr.INVALID),
        (dict(lst=[0], desc=dict(list_off=10000), list_ok=False), pr.INVALID),
        (dict(lst=[0, 10]), pr.INVALID),
        (dict(lst=[5]), pr.INVALID),
        (dict(lst=[1, 7]), pr.INVALID),
        (dict(lst=[4, 5]), pr.INVALID),                                        # judged behind a CLOSE as well
        (dict(lst=[0, 5], closed=1), pr.INVALID),                              # 1 before 2
        (dict(lst=[0, 2], closed=1), 0),                                       # 2 before 3
        (dict(lst=[6, 6, 6]), 0),
        (dict(lst=[]), 0),
        (dict(lst=[2]), pr.CONTROL),                                           # row 3
        (dict(lst=[3, 2]), pr.CONTROL),                                        # 3 before 4
        (dict(lst=[4, 2]), pr.CONTROL),
        (dict(lst=[3]), pr.DECLINED),                                          # row 4
        (dict(lst=[8]), pr.DECLINED),
        (dict(lst=[4, 3]), pr.DECLINED),
        (dict(lst=[0, 3], open=1), pr.DECLINED),                               # 4 before 5
        (dict(lst=[1, 0], open=1), pr.SEQUENCE),                               # row 5
        (dict(lst=[0], open=1, out_cap=1), pr.SEQUENCE),                       # 5 before 6
        (dict(lst=[0, 1], out_cap=108), pr.CAPACITY),                          # row 6
        (dict(lst=[0, 1], out_cap=109), 0),
        (dict(lst=[0, 1], out_cap=0), pr.CAPACITY),
    ]
    subs = []
    for k, (s, _) in enumerate(cases):
        subs.append(dict(conn=2 * k, lst=good))
        subs.append(dict(s, conn=2 * k + 1))
    for s in subs:                                         # a list_len by hand must not be taken for the model's list
        if "list_len" in s.get("desc", {}) and "list_ok" not in s:
            s["model_lst"] = [0] * s["desc"]["list_len"]
    pc = PConns(cuda, len(subs))
    for s in subs:
        if s.get("closed"):
            pc.preset(s["conn"], st=dict(close_sent=1))
        if s.get("open"):
            pc.preset(s["conn"], tx=dict(last_msg_not_fin=1))
    p = Pub(cuda, pc, recs, bufs, subs, SMALL)
    for s in subs:
        if "model_lst" in s:
            s["lst"] = s["model_lst"]
    outs = p.expect()
    p.launch(ctx)
    torch.cuda.synchronize()
    p.check()
    pc.check()
    assert statuses(outs[1::2]) == [want for _, want in cases]
    assert statuses(outs[0::2]) == [0] * len(cases) and all(o["bytes"] == outs[0]["bytes"] for o in outs[0::2])
    assert outs[2 * 22 + 1]["res"] == tr.refusal(pr.CAPACITY, 2, 109)
    # a record that names a base passed as NULL: refused; a list that names none such is written
    pc = PConns(cuda, 3)
    outs, _ = run(ctx, cuda, pc, recs, [bufs[0], None, bufs[2]],
                  [dict(conn=0, lst=[0, 1]), dict(conn=1, lst=[0, 9]), dict(conn=2, lst=[1])], SMALL)
    assert statuses(outs) == [0, pr.INVALID, 0]
    # without frame records: dev_frames NULL, every frame_cap 0
    pc = PConns(cuda, 2)
    p = Pub(cuda, pc, recs, bufs, [dict(conn=0, lst=[0, 1, 4], frame_cap=0), dict(conn=1, lst=[1], frame_cap=0)], SMALL)
    p.expect()
    p.launch(ctx, frames=False)
    torch.cuda.synchronize()
    p.check()
    pc.check()


# ------------------------------------------------------------------ 6. the largest region
def test_256_records_of_128_kib_from_a_shared_source(ctx, cuda):
    """One subscriber, 256 records of 128 KiB that overlap in one source (record k
    starts k bytes in): 256 * (128 KiB + 10) bytes, the largest region there is,
    checked by hash; the guards around it bytewise."""
    n, ln = 256, FULL
    bufs = [sources(10, ln + n + 16)[0], None, None]
    recs = pr.records([(BIN if k & 1 else TEXT, IN_DST, k, ln) for k in range(n)])
    total = n * (ln + 10)
    assert total == _lib.FWS_PUB_MAX_ITEMS * (_lib.FWS_TX_MULTI_MAX_SEND + 10) < 1 << 26
    pc = PConns(cuda, 1)
    p = Pub(cuda, pc, recs, bufs, [dict(conn=0, lst=list(range(n)), out_cap=total, frame_cap=n)], FULL, mis=(7, 0, 0))
    out = pr.predict(pc.tx[0], pc.st[0], recs, p.bufs, list(range(n)), out_cap=total)
    pc.tx[0] = out["tx"]
    assert out["res"]["status"] == 0 and out["res"]["out_len"] == total and len(out["bytes"]) == total
    p.launch(ctx)
    torch.cuda.synchronize()
    got = p.arena.cpu().numpy()
    o = p.subs[0]["out_off"]
    assert hashlib.sha256(got[o:o + total].tobytes()).digest() == hashlib.sha256(out["bytes"]).digest()
    assert got[:o].tobytes() == bytes([FILL]) * o and got[o + total:o + total + GUARD].tobytes() == bytes([FILL]) * GUARD
    fo = p.sec["frames"][0]
    assert got[fo:fo + n * FSZ].tobytes() == out["records"].tobytes()
    assert got[fo + n * FSZ:fo + (n + FRAME_GUARD) * FSZ].tobytes() == bytes([FILL]) * (FRAME_GUARD * FSZ)
    res = np.frombuffer(got[p.sec["res"][0]:][:RSZ].tobytes(), dtype=_lib.TX_RESULT)[0]
    assert {k: int(res[k]) for k in _lib.TX_RESULT.names} == out["res"]
    assert int(out["records"][-1]["hdr_off"]) == total - ln - 10
    pc.check()
    # one byte short: refused with the bytes needed, nothing written
    pc = PConns(cuda, 1)
    outs, _ = run(ctx, cuda, pc, recs, bufs, [dict(conn=0, lst=list(range(n)), out_cap=total - 1, frame_cap=0)], FULL)
    assert outs[0]["res"] == tr.refusal(pr.CAPACITY, n, total)


# ------------------------------------------------------------------ 7. decode -> join -> publish
def test_decode_join_publish_on_one_stream(ctx, cuda):
    """dev_joined zeroed, the flow decode, the join and the publish queued on one
    stream with nothing from the host in between, twice. Connection 0 sends a
    TEXT message cut across the two reads (delivered from the store in the
    second call), connection 1 a whole BIN message and a PING in each read,
    connection 2 nothing. All three subscribe to one list that names every slot
    of both reads' entry slices: what each receives is what JoinRef says the
    call delivered."""
    rng = random.Random(11)
    text = gj.cc.random_text(rng, 300)
    a = gj.frame(TEXT, text, key=gj.key(rng))
    bodies = [(gj.cc.payload(rng, 200), b"ping one"), (gj.cc.payload(rng, 77), b"ping two")]
    b = [gj.frame(BIN, body, key=gj.key(rng)) + gj.frame(PING, ping, key=gj.key(rng)) for body, ping in bodies]
    conns, jc, pc = fm.Conns(cuda, 3), gj.JConns(cuda, 3, 512), PConns(cuda, 3)
    calls = []
    for k, part in enumerate((a[:120], a[120:])):
        reads = [dict(wire=part, conn=0, msg_cap=8), dict(wire=b[k], conn=1, msg_cap=8)]
        m = fm.Flow(cuda, conns, reads)
        jn = gj.Join(cuda, m, jc)
        calls.append((m, jn))
    prepared = []
    for m, jn in calls:
        slots = [r["eb"] + j for r in m.reads for j in range(r["msg_cap"])]
        lst = torch.tensor(slots, dtype=torch.int32, device=cuda).view(torch.uint8)
        desc = np.zeros(3, dtype=_lib.PUB_SUB)
        for c in range(3):
            desc[c] = (256 + c * 1024, 1024 - 2 * GUARD, 2 * c, 0, len(slots), 0, 0)
        subs = torch.from_numpy(desc.view(np.uint8).copy()).to(cuda)
        out = torch.full((256 + 3 * 1024,), FILL, dtype=torch.uint8, device=cuda)
        res = torch.full((3 * RSZ + GUARD,), FILL, dtype=torch.uint8, device=cuda)
        prepared.append((len(slots), lst, subs, out, res))
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    for (m, jn), (n_slots, lst, subs, out, res) in zip(calls, prepared):
        # ---- the stream: zero, decode, join, publish; then the same for the second reads
        o, sz = jn.sec["joined"]
        jn.arena[o:o + sz].zero_()
        m.launch(ctx)
        jn.launch(ctx)
        rc = gpu.publish_messages(ctx, jn.arena[o:], sz // JSZ, m.arena, jc.store, m.arena, lst, n_slots, subs, 3,
                                  SMALL, out, None, res, pc.conns, pc.states, pc.n_dev, stream=stream)
        assert rc == 0
    torch.cuda.synchronize()
    for m, jn in calls:
        m.expect()
        m.check()
        jn.host_in[jn.sec["joined"][0]:][:jn.sec["joined"][1]] = 0
        jn.expect()
        jn.check()
    jc.check()
    conns.check()
    delivered = []
    for (m, jn), (n_slots, lst, subs, out, res) in zip(calls, prepared):
        want = [(op, 1, body) for i in range(2) for op, body, _ in jn.units(i)]
        delivered.append(want)
        need = sum(tr.hdr_len(len(body), False) + len(body) for _, _, body in want)
        raw = res.cpu().numpy().tobytes()
        got, r = out.cpu().numpy(), np.frombuffer(raw[:3 * RSZ], dtype=_lib.TX_RESULT)
        assert raw[3 * RSZ:] == bytes([FILL]) * GUARD
        for c in range(3):
            assert {k: int(r[c][k]) for k in _lib.TX_RESULT.names} == \
                dict(status=0, n_frames=len(want), out_len=need, last_msg_not_fin=0, pad=0, reserved=0), c
            o = 256 + c * 1024
            assert rr.walk_frames(got[o:o + need].tobytes()) == want, c
            assert got[o + need:o + 1024].tobytes() == bytes([FILL]) * (1024 - need), c
        assert got[:256].tobytes() == bytes([FILL]) * 256
        pc.tx = [dict(t, frames=t["frames"] + len(want), wire_bytes=t["wire_bytes"] + need) for t in pc.tx]
    assert delivered[0] == [(BIN, 1, bodies[0][0]), (PING, 1, bodies[0][1])]
    assert delivered[1] == [(TEXT, 1, text), (BIN, 1, bodies[1][0]), (PING, 1, bodies[1][1])]
    assert calls[1][1].outs[0]["records"][0]["where"] == IN_STORE
    pc.check()


# ------------------------------------------------------------------ 8. MessagePublisher
def test_message_publisher_equals_the_model_and_shares_a_senders_conns(ctx, cuda):
    rng = random.Random(12)
    messages = [(TEXT, b"hello, room"), (BIN, bytes(rng.getrandbits(8) for _ in range(5000))), (PING, b"tick"),
                (BIN, b""), (TEXT, bytes(rng.getrandbits(7) for _ in range(70000)))]
    n = 6
    sender = gpu.MessageSender(ctx, n, max_send=4096)
    pub = gpu.MessagePublisher(ctx, n, max_out=80000, conns=sender.conns)
    room = [0, 1, 2, 3]
    lists = {0: room, 1: room, 2: [4, 2], 3: list(room), 5: []}
    got = pub.publish(messages, lists)
    assert pub.lists_uploaded == 3 and pub.calls == 1

    def model(tx, st, lst, max_len=FULL):
        data = b"".join(p for _, p in messages)
        recs, at = [], 0
        for op, p in messages:
            recs.append((op, IN_DST, at, len(p)))
            at += len(p)
        return pr.predict(tx, st, pr.records(recs), (data, None, None), lst, max_len=max_len, out_cap=pub.out_slot)

    want = {c: model(pr.new_tx(), pr.new_state(), lst) for c, lst in lists.items()}
    assert got == {c: w["bytes"] for c, w in want.items()} and got[5] == b"" and len(got[2]) == 70010 + 6
    for c in range(n):
        tx = gpu.read_tx_conn(sender.conns, c)
        assert int(tx["frames"]) == (want[c]["tx"]["frames"] if c in want else 0)
    # the sender opens a message on connection 0: the publisher's data is refused there, a PING goes through
    first = sender.send({0: (TEXT, b"part one, ", False)}, masked=False)
    with pytest.raises(gpu.FwsError) as e:
        pub.publish(messages, {0: [2, 0], 1: [0]})
    assert e.value.code == _lib.FWS_ERR_SEQUENCE
    ping = pub.publish(messages, {0: [2]})
    last = sender.send({0: (TEXT, b"part two", True)}, masked=False)
    after = pub.publish(messages, {0: [0]})
    units, open_ = rr.messages(rr.walk_frames(first[0] + ping[0] + last[0] + after[0]))
    assert open_ is None and units == [(PING, b"tick"), (TEXT, b"part one, part two"), (TEXT, b"hello, room")]
    # a CLOSE: the connection gets nothing more; a publisher of its own has zeroed states
    bye = [(CLOSE, bytes([0x03, 0xE9]))]
    solo = gpu.MessagePublisher(ctx, 2, max_out=64)
    assert solo.publish(bye + messages[:1], {1: [1, 0, 1]}) == {1: want[0]["bytes"][:13] + b"\x88\x02\x03\xe9"}
    assert solo.publish(messages, {1: [0], 0: [0]}) == {1: b"", 0: want[0]["bytes"][:13]}
    assert int(gpu.read_reply_state(solo.states, 1)["close_sent"]) == 1
    with pytest.raises(gpu.FwsError) as e:
        solo.publish(messages, {0: [1]})                  # 5,004 bytes into a region of 64
    assert e.value.code == _lib.FWS_ERR_CAPACITY
