"""GPU parity of fws_gpu_encode_messages_multi: the sends of many connections cut
into frames and encoded in one launch, sequenced by a state in device memory.

The oracle is txmulti_ref.predict (one orc.OrcTx.frame() per fragment);
test_tx_multi_cpu.py holds it against the reference's recorded frames. Every
call is checked byte for byte: the whole output buffer (pre-filled with 0xEE;
every byte outside [out_off, out_off + out_len) must still be 0xEE -- the rest
of each region, the gaps between regions, a 64-byte guard band at either end),
every fws_tx_result, the whole frame-record buffer (records past the count and
the guard records stay 0xEE) and the connections' 32-byte states, which lie in
an array whose odd records are guards. All comparisons are exact."""
import random

import numpy as np
import pytest
import torch

import txmulti_ref as tr
from flashws_amd import _lib, gpu
from txmulti_ref import BIN, CAPACITY, CLOSE, CONTROL, DECLINED, INVALID, PING, PONG, TEXT

pytestmark = pytest.mark.gpu

FILL, GUARD = 0xEE, 64
fill = bytes([FILL])
CSZ, SSZ, RSZ, FSZ = (_lib.TX_CONN.itemsize, _lib.TX_SEND.itemsize, _lib.TX_RESULT.itemsize,
                      _lib.FRAME_INFO.itemsize)
SMALL, FULL = 16 << 10, _lib.FWS_TX_MULTI_MAX_SEND       # the kernel forms' bounds (max_len)


def payload_of(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


class Conns:
    """The connections of a test: their states on the device -- record 2c is
    connection c's, the odd records are guards -- and the model's states."""

    def __init__(self, cuda, n, open_=None):
        self.n, self.n_dev = n, 2 * n
        self.ref = [tr.new_state() for _ in range(n)]
        host = np.full(self.n_dev * CSZ + GUARD, FILL, dtype=np.uint8)
        for c in range(n):
            if open_ is not None:
                self.ref[c]["last_msg_not_fin"] = int(open_[c])
            host[2 * c * CSZ:(2 * c + 1) * CSZ] = np.frombuffer(tr.state_bytes(self.ref[c]), dtype=np.uint8)
        self.t = torch.from_numpy(host).to(cuda)

    def image(self):
        raw = bytearray(fill * (self.n_dev * CSZ + GUARD))
        for c in range(self.n):
            raw[2 * c * CSZ:(2 * c + 1) * CSZ] = tr.state_bytes(self.ref[c])
        return bytes(raw)

    def check(self, got=None, want=None):
        got = self.t.cpu().numpy().tobytes() if got is None else got
        want = self.image() if want is None else want
        if got != want:
            for c in range(self.n):
                rec = np.frombuffer(got[2 * c * CSZ:(2 * c + 1) * CSZ], dtype=_lib.TX_CONN)[0]
                ref = np.frombuffer(want[2 * c * CSZ:(2 * c + 1) * CSZ], dtype=_lib.TX_CONN)[0]
                for k in _lib.TX_CONN.names:
                    assert int(rec[k]) == int(ref[k]), ("state", c, k, int(rec[k]), int(ref[k]))
                assert got[(2 * c + 1) * CSZ:(2 * c + 2) * CSZ] == fill * CSZ, ("the guard behind state", c)
            assert got == want, "the guard band behind the states"


def send(payload, conn, ft=BIN, last=1, masked=1, key=0x1234ABCD, max_frame=0, shift=0, out_cap=None, frame_cap=None,
         out_shift=0, conn_dev=None, slack=0):
    """A send of a test. shift: the payload's source misalignment; out_cap None:
    the bytes needed + slack; out_shift: added to out_off (a misaligned region);
    conn_dev: the descriptor's conn when it is not the connection's record."""
    return dict(payload=payload, conn=conn, ft=ft, last=last, masked=masked, key=key, max_frame=max_frame,
                shift=shift, out_cap=out_cap, frame_cap=frame_cap, out_shift=out_shift, conn_dev=conn_dev, slack=slack)


class Call:
    """One call: the buffers laid out, the model's prediction for every send
    (which advances the connections' model states), the launch, the check."""

    def __init__(self, cuda, conns, sends, max_len=None):
        self.conns, self.sends, self.n = conns, sends, len(sends)
        self.max_len = max_len if max_len is not None else max(1, max(len(s["payload"]) for s in sends))
        desc = np.zeros(self.n, dtype=_lib.TX_SEND)
        src = bytearray(fill * 32)
        out_pos, frame_pos = GUARD, 1
        self.outs = []
        for i, s in enumerate(sends):
            p, masked = s["payload"], bool(s["masked"])
            while len(src) % 16 != s["shift"] % 16:
                src += fill
            src_off = len(src)
            src += p + fill
            need = sum(tr.hdr_len(ln, masked) + ln for _, ln in tr.slices(len(p), s["max_frame"], bool(s["ft"] & 8)))
            cap = s["out_cap"] if s["out_cap"] is not None else need + s["slack"]
            k = len(tr.slices(len(p), s["max_frame"], bool(s["ft"] & 8)))
            fcap = s["frame_cap"] if s["frame_cap"] is not None else min(k, 256) + 1
            bad_conn = s["conn_dev"] is not None
            state = conns.ref[s["conn"]]
            out = tr.predict(state, p, s["ft"], s["last"], masked=masked, key=s["key"], max_frame=s["max_frame"],
                             out_cap=cap, frame_cap=fcap, max_len=self.max_len, out_off=out_pos + s["out_shift"],
                             conn_ok=not bad_conn)
            conns.ref[s["conn"]] = out["state"]
            out.update(out_off=out_pos + s["out_shift"], cap=cap, frame_base=frame_pos, frame_cap=fcap)
            self.outs.append(out)
            d = desc[i]
            d["src_off"], d["out_off"], d["len"], d["out_cap"] = src_off, out["out_off"], len(p), cap
            d["conn"] = s["conn_dev"] if bad_conn else 2 * s["conn"]
            d["max_frame"], d["key"], d["frame_type"], d["last"], d["masked"] = (s["max_frame"], s["key"], s["ft"],
                                                                                 s["last"], s["masked"])
            d["frame_base"], d["frame_cap"] = frame_pos, fcap
            out_pos = (out_pos + cap + 15 & ~15) + 16 * (1 + i % 3)       # a gap of 16..48 bytes behind each region
            frame_pos += fcap + 1                                         # a guard record behind each slice
        self.out_size, self.n_frames_buf = out_pos + GUARD, frame_pos
        src += fill * 32
        self.desc = desc
        self.src = torch.from_numpy(np.frombuffer(bytes(src), dtype=np.uint8).copy()).to(cuda)
        self.d_sends = torch.from_numpy(desc.view(np.uint8).copy()).to(cuda)
        self.out = torch.full((self.out_size,), FILL, dtype=torch.uint8, device=cuda)
        self.frames = torch.full((self.n_frames_buf * FSZ,), FILL, dtype=torch.uint8, device=cuda)
        self.res = torch.full((self.n * RSZ + GUARD,), FILL, dtype=torch.uint8, device=cuda)
        self.states_after = conns.image()

    def launch(self, ctx, stream=None, frames=True):
        rc = gpu.encode_messages_multi(ctx, self.out, self.src, self.d_sends, self.n, self.max_len,
                                       self.frames if frames else None, self.res, self.conns.t, self.conns.n_dev,
                                       stream=stream)
        assert rc == 0, rc

    def images(self):
        out = bytearray(fill * self.out_size)
        frames = bytearray(fill * (self.n_frames_buf * FSZ))
        for o in self.outs:
            out[o["out_off"]:o["out_off"] + len(o["bytes"])] = o["bytes"]
            rec = o["records"].tobytes()
            frames[o["frame_base"] * FSZ:o["frame_base"] * FSZ + len(rec)] = rec
        return bytes(out), bytes(frames)

    def check(self):
        res_raw = self.res.cpu().numpy().tobytes()
        assert res_raw[self.n * RSZ:] == fill * GUARD, "the guard behind the results"
        res = np.frombuffer(res_raw[:self.n * RSZ], dtype=_lib.TX_RESULT)
        for i, o in enumerate(self.outs):
            for k in _lib.TX_RESULT.names:
                assert int(res[i][k]) == o["res"][k], ("result", i, k, int(res[i][k]), o["res"][k])
        want_out, want_frames = self.images()
        got = self.got = self.out.cpu().numpy().tobytes()
        if got != want_out:
            at = next(j for j in range(len(got)) if got[j] != want_out[j])
            i = max((i for i, o in enumerate(self.outs) if o["out_off"] <= at), default=0)
            o, s = self.outs[i], self.sends[i]
            raise AssertionError(("out", "send", i, "byte", at - o["out_off"], "of", len(o["bytes"]), "cap", o["cap"],
                                  "len", len(s["payload"]), "max_frame", s["max_frame"], "masked", s["masked"],
                                  "shift", s["shift"], "got", got[at], "want", want_out[at]))
        got_frames = self.frames.cpu().numpy().tobytes()
        if got_frames != want_frames:
            for i, o in enumerate(self.outs):
                reg = got_frames[o["frame_base"] * FSZ:(o["frame_base"] + o["frame_cap"] + 1) * FSZ]
                recs = np.frombuffer(reg[:len(o["records"]) * FSZ], dtype=_lib.FRAME_INFO)
                for j, r in enumerate(o["records"]):
                    for k in _lib.FRAME_INFO.names:
                        assert int(recs[j][k]) == int(r[k]), ("record", i, j, k, int(recs[j][k]), int(r[k]))
                assert reg[len(o["records"]) * FSZ:] == fill * (len(reg) - len(o["records"]) * FSZ), \
                    ("records past the count", i)
            assert got_frames == want_frames
        return res


def run(ctx, cuda, conns, sends, max_len=None):
    """One call, checked in full: returns (the model's outputs, the call)."""
    m = Call(cuda, conns, sends, max_len)
    m.launch(ctx)
    torch.cuda.synchronize()
    m.check()
    conns.check()
    return m.outs, m


LENGTHS = [0, 1, 125, 126, 127, 65535, 65536, 65537, 131072]


@pytest.mark.parametrize("base", [0, 2])
def test_every_length_form_masked_and_unmasked(ctx, cuda, base):
    """18 sends in one call: every header form and its edges up to the largest
    send; the source misalignments of both calls sweep 0..19."""
    conns = Conns(cuda, 18)
    sends = [send(payload_of(100 + i, n), i, ft=TEXT + i % 2, masked=i < 9, key=0xA1B2C3D4 + 77 * i,
                  shift=base + i, slack=i % 5)
             for i, n in enumerate(LENGTHS + LENGTHS)]
    outs, m = run(ctx, cuda, conns, sends, FULL)
    assert [o["res"]["status"] for o in outs] == [0] * 18 and m.max_len == FULL
    assert [int(o["records"][0]["hdr_len"]) for o in outs] == [6, 6, 6, 8, 8, 8, 14, 14, 14, 2, 2, 2, 4, 4, 4, 10, 10, 10]
    assert outs[8]["res"]["out_len"] == 131072 + 14 and conns.ref[8]["wire_bytes"] == 131072 + 14


def fragmentation_sends():
    sends, rng = [], random.Random(5)
    for m in (1, 2, 3, 13, 16, 125, 126, 127, 4096):
        for k in (1, 2, 3, 17):
            for n in (k * m - 1, k * m, k * m + 1):
                for masked in (1, 0):
                    i = len(sends)
                    sends.append(send(payload_of(1000 + i, n), i, ft=TEXT + i % 2, last=rng.randrange(2), masked=masked,
                                      key=rng.getrandbits(32), max_frame=m, shift=rng.randrange(16),
                                      slack=rng.randrange(20)))
    return sends


@pytest.mark.parametrize("form", ["full", "small"])
def test_fragmentation(ctx, cuda, form):
    """Sends cut at, before and behind a multiple of max_frame, from 3-byte frames
    (several whole frames in one 16-B chunk) to 4 KiB ones; half the connections
    have a message open, so frame 0 is a continuation there."""
    sends = fragmentation_sends()
    if form == "small":
        sends = [dict(s, conn=i) for i, s in enumerate(s for s in sends if len(s["payload"]) <= SMALL)]
    assert len(sends) == (216 if form == "full" else 210)
    conns = Conns(cuda, len(sends), open_=[i % 4 < 2 for i in range(len(sends))])
    outs, m = run(ctx, cuda, conns, sends, FULL if form == "full" else SMALL)
    several = 0
    for s, o in zip(sends, outs):
        n, mf = len(s["payload"]), s["max_frame"]
        k = max(1, -(-n // mf))
        assert o["res"]["status"] == 0 and o["res"]["n_frames"] == k == len(o["records"])
        # the keys follow FWS_TX_FRAG_KEY, in the records and on the wire
        got = m.got[o["out_off"]:o["out_off"] + o["res"]["out_len"]]
        for j, r in enumerate(o["records"]):
            want = _lib.FWS_TX_FRAG_KEY(s["key"], j) if s["masked"] else 0
            assert int(r["key"]) == want
            if s["masked"]:
                at = int(r["hdr_off"]) + int(r["hdr_len"]) - 4
                assert int.from_bytes(got[at:at + 4], "little") == want, (n, mf, j)
        several += k >= 3 and mf + tr.hdr_len(mf, s["masked"]) <= 5
    assert several >= 8                                   # chunks holding three whole frames and more


def test_frame_limits(ctx, cuda):
    """Exactly FWS_TX_MULTI_MAX_FRAMES frames are encoded; one more is declined
    and leaves the region, the records and the state alone."""
    conns = Conns(cuda, 4, open_=[0, 1, 1, 0])
    sends = [send(payload_of(7 + i, n), i, masked=masked, max_frame=1, last=i % 2, shift=3 + i, out_cap=4096)
             for i, (n, masked) in enumerate([(256, 1), (257, 1), (256, 0), (257, 0)])]
    outs, _ = run(ctx, cuda, conns, sends)
    assert [o["res"]["status"] for o in outs] == [0, DECLINED, 0, DECLINED]
    assert [o["res"]["n_frames"] for o in outs] == [256, 0, 256, 0]
    assert outs[0]["res"]["out_len"] == 256 * 7 and outs[2]["res"]["out_len"] == 256 * 3
    assert [c["frames"] for c in conns.ref] == [256, 0, 256, 0]


def test_every_tail_length(ctx, cuda):
    """Payloads 0..40 with both header kinds: out_len % 16 takes every value, and
    the tail is stored partially -- the region's own spare bytes stay untouched."""
    conns = Conns(cuda, 82)
    sends = [send(payload_of(300 + i, i % 41), i, masked=i < 41, shift=i % 16, slack=40) for i in range(82)]
    outs, _ = run(ctx, cuda, conns, sends)
    assert {o["res"]["out_len"] % 16 for o in outs[:41]} == set(range(16))
    assert {o["res"]["out_len"] % 16 for o in outs[41:]} == set(range(16))


def test_capacity(ctx, cuda):
    """out_cap = the bytes needed is enough, one byte less refuses the send with
    the count in out_len; an empty send still needs its header."""
    shapes = [(0, 0, 1), (0, 0, 0), (5, 0, 1), (126, 0, 1), (300, 100, 1), (301, 100, 0), (70000, 0, 1),
              (70000, 4096, 1), (16, 1, 1)]
    sends = []
    for n, mf, masked in shapes:
        need = sum(tr.hdr_len(ln, masked) + ln for _, ln in tr.slices(n, mf))
        for cap in (need, need - 1):
            i = len(sends)
            sends.append(send(payload_of(500 + i, n), i, masked=masked, max_frame=mf, out_cap=cap, shift=i))
    sends.append(send(b"", len(sends), masked=1, out_cap=0))
    sends.append(send(b"", len(sends), masked=0, out_cap=0))
    conns = Conns(cuda, len(sends), open_=[i % 3 == 0 for i in range(len(sends))])
    before = [dict(s) for s in conns.ref]
    outs, _ = run(ctx, cuda, conns, sends)
    for i, o in enumerate(outs[:-2]):
        assert o["res"]["status"] == (0 if i % 2 == 0 else CAPACITY), i
        assert o["res"]["out_len"] == outs[i & ~1]["res"]["out_len"] and o["res"]["n_frames"] >= 1
        if i % 2:
            assert conns.ref[i] == before[i] and o["bytes"] == b""
    assert [(o["res"]["status"], o["res"]["out_len"], o["res"]["n_frames"]) for o in outs[-2:]] == \
        [(CAPACITY, 6, 1), (CAPACITY, 2, 1)]


def test_sequencing_over_queued_calls(ctx, cuda):
    """Five calls queued on one stream, one synchronisation at the end: TEXT
    last = 0, a PING, BIN last = 0 (a continuation), last = 1, TEXT last = 1. The
    state after each call is read back from a copy made on the stream. The PING
    has last = 0 and carries FIN = 0, the oracle's rule."""
    conns = Conns(cuda, 2)
    steps = [(TEXT, 0, b"first part ", 4), (PING, 0, b"are you there", 0), (BIN, 0, payload_of(1, 700), 256),
             (TEXT, 1, b" and the end", 0), (TEXT, 1, b"a new message", 5)]
    other = [(PING, 1, b"", 0), (BIN, 1, payload_of(2, 300), 128), (CLOSE, 1, b"\x03\xe8bye", 0),
             (BIN, 0, payload_of(3, 40), 16), (PONG, 0, b"x" * 125, 0)]
    calls, snaps, images = [], [], []
    for (ft, last, p, mf), (ft2, last2, p2, mf2) in zip(steps, other):
        calls.append(Call(cuda, conns, [send(p, 0, ft=ft, last=last, max_frame=mf, key=0x0BADF00D, shift=5),
                                        send(p2, 1, ft=ft2, last=last2, max_frame=mf2, masked=0, shift=9)]))
        images.append(calls[-1].states_after)
    stream = torch.cuda.current_stream()
    for m in calls:
        m.launch(ctx, stream=stream)
        snaps.append(conns.t.clone())                     # a copy on the stream, no synchronisation
    stream.synchronize()
    for m, snap, image in zip(calls, snaps, images):
        m.check()
        conns.check(snap.cpu().numpy().tobytes(), image)
    conns.check()
    first = [(int(m.outs[0]["records"][0]["opcode"]), int(m.outs[0]["records"][-1]["fin"])) for m in calls]
    assert first == [(TEXT, 0), (PING, 0), (0, 0), (0, 1), (TEXT, 1)]
    assert [m.outs[0]["res"]["last_msg_not_fin"] for m in calls] == [1, 1, 1, 0, 0]
    assert [m.outs[1]["res"]["last_msg_not_fin"] for m in calls] == [0, 0, 0, 1, 1]
    assert conns.ref[0]["frames"] == 3 + 1 + 3 + 1 + 3


def test_isolation_of_refused_sends(ctx, cuda):
    """One call with two good sends and every per-send refusal: each refused send
    has its status and nothing else is written for it; the good ones are exact."""
    conns = Conns(cuda, 9, open_=[1] * 9)
    sends = [send(payload_of(1, 5000), 0, max_frame=1000, shift=1),
             send(payload_of(2, 5000), 1, out_cap=5007),                        # needs 5008
             send(payload_of(3, 126), 2, ft=PING),
             send(payload_of(4, 9000), 3),                                      # len > max_len
             send(payload_of(5, 100), 4, out_shift=8),
             send(payload_of(6, 100), 5, conn_dev=18),                          # conn >= n_conns
             send(payload_of(7, 100), 6, ft=3),
             send(payload_of(8, 100), 7, ft=0),
             send(payload_of(9, 8192), 8, masked=0, max_frame=4096, last=0, shift=15)]
    outs, _ = run(ctx, cuda, conns, sends, max_len=8192)
    assert [o["res"]["status"] for o in outs] == [0, CAPACITY, CONTROL, DECLINED, INVALID, INVALID, INVALID, INVALID,
                                                  0]
    assert outs[1]["res"]["out_len"] == 5008
    assert [c["frames"] for c in conns.ref] == [5, 0, 0, 0, 0, 0, 0, 0, 2]


def test_both_kernel_forms_write_the_same(ctx, cuda):
    """max_len 16384 and 16385 select the two forms: the same sends give the same
    outputs, records, results and states."""
    rng = random.Random(21)
    sends = [send(payload_of(40 + i, rng.choice([0, 1, 15, 16, 17, 1000, 4095, 16384, rng.randrange(16385)])), i,
                  ft=rng.choice([TEXT, BIN]), last=rng.randrange(2), masked=rng.randrange(2), key=rng.getrandbits(32),
                  max_frame=rng.choice([0, 0, 64, 100, 1024, 5000]), shift=rng.randrange(16), slack=rng.randrange(30))
             for i in range(48)]
    sends.append(send(payload_of(99, 16384), 48, masked=1, shift=7))
    seen = []
    for max_len in (SMALL, SMALL + 1):
        conns = Conns(cuda, len(sends), open_=[i % 2 for i in range(len(sends))])
        outs, m = run(ctx, cuda, conns, sends, max_len)
        assert all(o["res"]["status"] == 0 for o in outs)
        seen.append((m.got, m.frames.cpu().numpy().tobytes(), m.res.cpu().numpy().tobytes(),
                     conns.t.cpu().numpy().tobytes()))
    assert seen[0] == seen[1]


def test_many_connections(ctx, cuda):
    """512 sends of 0..2 KiB in one call over 512 connections with random prior
    state, random max_frame (or none), mask bit and `last`; the records of every
    third send are cut short by frame_cap."""
    rng = random.Random(33)
    n = 512
    conns = Conns(cuda, n, open_=[rng.randrange(2) for _ in range(n)])
    order = list(range(n))
    rng.shuffle(order)
    sends = []
    for i in range(n):
        ln = rng.randrange(2049)
        mf = rng.choice([0, 0, 9, 50, 126, 500, 2048])
        ft = rng.choice([TEXT, BIN, BIN, PING]) if ln <= 125 else rng.choice([TEXT, BIN])
        sends.append(send(payload_of(2000 + i, ln), order[i], ft=ft, last=rng.randrange(2), masked=rng.randrange(2),
                          key=rng.getrandbits(32), max_frame=mf, shift=rng.randrange(16), slack=rng.randrange(33),
                          frame_cap=rng.randrange(3) if i % 3 == 0 else None))
    outs, _ = run(ctx, cuda, conns, sends)
    assert all(o["res"]["status"] == 0 for o in outs)
    assert any(len(o["records"]) < o["res"]["n_frames"] for o in outs)
    assert sum(c["frames"] for c in conns.ref) == sum(o["res"]["n_frames"] for o in outs) > 2 * n


def test_null_frames_with_no_frame_cap(ctx, cuda):
    """dev_frames may be NULL when every frame_cap is 0."""
    conns = Conns(cuda, 3)
    m = Call(cuda, conns, [send(payload_of(60 + i, 100 * i), i, max_frame=64, frame_cap=0) for i in range(3)])
    m.launch(ctx, frames=False)
    torch.cuda.synchronize()
    m.check()
    conns.check()


def test_round_trip_through_the_flow_decode(ctx, cuda):
    """8 connections send masked messages of 0..20 KiB in frames of 1000 bytes;
    the out regions go to fws_gpu_decode_messages_flow as 8 reads: the decoded
    messages are the payloads with their opcodes, and the frame records of both
    calls are equal field by field."""
    n = 8
    rng = random.Random(8)
    lens = [0, 1, 999, 1000, 1001, 20 << 10] + [rng.randrange(20 << 10) for _ in range(2)]
    conns = Conns(cuda, n)
    sends = [send(payload_of(700 + i, lens[i]), i, ft=TEXT + i % 2, last=1, masked=1, key=rng.getrandbits(32),
                  max_frame=1000, shift=i) for i in range(n)]
    outs, tx = run(ctx, cuda, conns, sends)
    slot, fcap, mcap = 32 << 10, 32, 4
    reads = np.zeros(n, dtype=_lib.MSG_READ)
    for i, o in enumerate(outs):
        reads[i] = (o["out_off"], i * slot, i * slot, o["res"]["out_len"], i, slot, slot, i * fcap, fcap, i * mcap,
                    mcap, 0)
    u8 = dict(dtype=torch.uint8, device=cuda)
    d_reads = torch.from_numpy(reads.view(np.uint8).copy()).to(cuda)
    frames, msgs = torch.zeros(n * fcap * FSZ, **u8), torch.zeros(n * mcap * _lib.MSG_INFO.itemsize, **u8)
    dst, ctl = torch.zeros(n * slot, **u8), torch.zeros(n * slot, **u8)
    res = torch.zeros(n * _lib.DECODE_RESULT.itemsize, **u8)
    mres = torch.zeros(n * _lib.MSG_RESULT.itemsize, **u8)
    flows = torch.zeros(n * _lib.MSG_FLOW.itemsize, **u8)
    rc = gpu.decode_messages_flow(ctx, tx.out, d_reads, n, max(o["res"]["out_len"] for o in outs), frames, msgs, dst,
                                  ctl, res, mres, flows, n)
    assert rc == 0
    torch.cuda.synchronize()
    assert tx.out.cpu().numpy().tobytes() == tx.got          # the decode left the wire alone
    mres = np.frombuffer(mres.cpu().numpy().tobytes(), dtype=_lib.MSG_RESULT)
    msgs = np.frombuffer(msgs.cpu().numpy().tobytes(), dtype=_lib.MSG_INFO)
    rx = np.frombuffer(frames.cpu().numpy().tobytes(), dtype=_lib.FRAME_INFO)
    dst = dst.cpu().numpy()
    for i, (s, o) in enumerate(zip(sends, outs)):
        assert int(mres[i]["status"]) == 0 and int(mres[i]["n_msgs"]) == 1, i
        e = msgs[i * mcap]
        assert int(e["opcode"]) == s["ft"] and int(e["len"]) == len(s["payload"])
        assert dst[i * slot + int(e["off"]):i * slot + int(e["off"]) + int(e["len"])].tobytes() == s["payload"]
        k = o["res"]["n_frames"]
        assert k == max(1, -(-len(s["payload"]) // 1000)) and int(e["n_data_frames"]) == k
        for j in range(k):
            for f in _lib.FRAME_INFO.names:
                assert int(rx[i * fcap + j][f]) == int(o["records"][j][f]), (i, j, f)


def test_graph_capture_and_replay(cuda):
    """One captured call (TEXT, last = 0, nothing else in the graph) replayed
    twice: the state chains the replays, so the second replay's frame is a
    continuation and the connection has sent two frames."""
    c = gpu.Ctx(0)                                        # (no reserve: the call has no workspace)
    try:
        p = payload_of(5, 3000)
        warm = Call(cuda, Conns(cuda, 1), [send(p, 0)])    # the kernel is loaded before the capture
        warm.launch(c)
        conns = Conns(cuda, 1)
        m = Call(cuda, conns, [send(p, 0, ft=TEXT, last=0, key=0x600DCAFE, shift=3)])
        first = m.outs[0]
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            m.launch(c)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        m.check()
        conns.check()
        assert int(first["records"][0]["opcode"]) == TEXT and conns.ref[0]["frames"] == 1
        # the second replay: the model's next send from the state the first one left
        again = Call(cuda, conns, [send(p, 0, ft=TEXT, last=0, key=0x600DCAFE, shift=3)])
        m.outs, m.states_after = again.outs, again.states_after
        m.out.fill_(FILL)
        g.replay()
        torch.cuda.synchronize()
        m.check()
        conns.check()
        assert int(m.outs[0]["records"][0]["opcode"]) == 0 and int(m.outs[0]["records"][0]["fin"]) == 0
        state = gpu.read_tx_conn(conns.t, 0)
        assert int(state["frames"]) == 2 and int(state["last_msg_not_fin"]) == 1
        assert int(state["wire_bytes"]) == 2 * (3000 + 8)
    finally:
        torch.cuda.synchronize()
        c.close()


def test_message_sender_streams_a_large_message(ctx, cuda):
    """MessageSender: a 300 KiB masked message in frames of 4096 bytes goes out in
    three internal calls and equals the model's bytes for the same pieces and
    keys; two other connections are served in the same send."""
    tx = gpu.MessageSender(ctx, 4, 128 << 10)
    big, small, ping = payload_of(1, 300 << 10), payload_of(2, 5000), b"ping!"
    keys = {0: 0x01020304, 2: 0xCAFEBABE, 3: 0x0F0E0D0C}
    got = tx.send({2: (BIN, big, 1), 0: (TEXT, small, 0), 3: (PING, ping, 1)}, max_frame=4096, keys=keys)
    assert tx.calls == 3
    assert [(o, ln) for o, ln, _ in tx.pieces[2]] == [(0, 128 << 10), (128 << 10, 128 << 10), (256 << 10, 44 << 10)]
    assert [k for _, _, k in tx.pieces[2]] == [_lib.FWS_TX_FRAG_KEY(keys[2], 32 * i) for i in range(3)]
    want = {}
    for c, (ft, p, last) in {2: (BIN, big, 1), 0: (TEXT, small, 0), 3: (PING, ping, 1)}.items():
        state, wire = tr.new_state(), b""
        for i, (o, ln, key) in enumerate(tx.pieces[c]):
            out = tr.predict(state, p[o:o + ln], ft, bool(last) and i + 1 == len(tx.pieces[c]), masked=True, key=key,
                             max_frame=4096)
            assert out["res"]["status"] == 0
            state, wire = out["state"], wire + out["bytes"]
        want[c] = (wire, state)
    for c in (0, 2, 3):
        assert got[c] == want[c][0], c
        assert gpu.read_tx_conn(tx.conns, c).tobytes() == tr.state_bytes(want[c][1]), c
    assert int(gpu.read_tx_conn(tx.conns, 2)["frames"]) == 75 and int(gpu.read_tx_conn(tx.conns, 1)["frames"]) == 0
    # the state stays on the device: the next send of connection 0 continues its open message
    more = tx.send({0: (TEXT, b"the rest", 1)}, keys={0: 5})
    assert more[0][0] == 0x80 and int(gpu.read_tx_conn(tx.conns, 0)["last_msg_not_fin"]) == 0
