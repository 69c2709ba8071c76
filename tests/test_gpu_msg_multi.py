"""GPU parity of fws_gpu_decode_messages_multi: the reads of many connections
decoded into messages in one launch, one workgroup per read.

The oracle is RefConn of test_gpu_msg_carry.py, one per connection: for read r
everything the call writes must be what fws_gpu_decode_messages_carry writes for
the same bytes, capacities and carry. Every call lays all reads' buffers out in
one device arena -- wire, dst, ctl, frame slice, entry slice, each followed by
guard bytes; the result arrays and the descriptors behind them; the carries in
an array whose odd records are guards no read names -- and checks, per read: the
wire unchanged, every guard, every fws_msg_result / fws_msg_info / fws_msg_carry
field, dst and ctl, the whole fws_decode_result and the frame records against
the reference parse. All comparisons are exact."""
import random
import struct

import numpy as np
import pytest
import torch

import test_gpu_msg_carry as cc
from flashws_amd import _lib, gpu
from test_gpu_msg_carry import (BIN, CONT, FILL, GUARD, NONE, PING, PONG, TEXT, RefConn, check_carry, frame,
                                new_carry, random_cuts, random_stream, twelve_frames, whole)

pytestmark = pytest.mark.gpu

DECLINED, INVALID = _lib.FWS_ERR_DECLINED, _lib.FWS_ERR_INVALID
SMALL, FULL = 16 << 10, _lib.FWS_MSG_MULTI_MAX_READ      # max_len of the two kernel forms
FSZ, ESZ = _lib.FRAME_INFO.itemsize, _lib.MSG_INFO.itemsize
DSZ, RSZ, CSZ = _lib.DECODE_RESULT.itemsize, _lib.MSG_RESULT.itemsize, _lib.MSG_CARRY.itemsize
FRAME_GUARD, ENTRY_GUARD = 3, 2                           # guard records behind a slice (72 / 64 bytes)
fill = bytes([FILL])


def align(n, a):
    return (n + a - 1) // a * a


def ref_decode_result(wire, cap):
    """fws_decode_result and the frame records of the reference parse."""
    frames, pstatus = cc.ref_parse(wire)
    n = len(wire)
    pos = frames[-1]["hdr_off"] + frames[-1]["hdr_len"] + frames[-1]["plen"] if frames else 0
    r = dict(status=pstatus, n_frames=len(frames), consumed=0, err_off=0, carry_unread=0, carry_hdr_len=0,
             n_survivors=len(frames))
    if pstatus:
        r["err_off"] = r["consumed"] = pos
    elif pos > n:
        r["carry_unread"], r["consumed"] = pos - n, n
    elif pos < n:
        r["carry_hdr_len"], r["consumed"] = n - pos, pos
    else:
        r["consumed"] = n
    if not pstatus and len(frames) > cap:
        r["status"] = _lib.FWS_ERR_CAPACITY
    recs = np.zeros(min(len(frames), cap), dtype=_lib.FRAME_INFO)
    for i in range(len(recs)):
        f = frames[i]
        recs[i] = (f["hdr_off"], f["plen"], int.from_bytes(bytes(f["key"]), "little"), f["op"], f["fin"],
                   f["hdr_len"], 1 if f["trunc"] else 0)
    return r, recs.tobytes()


class Conns:
    """The connections of a test: their carries on the device -- record 2c is
    connection c's, the odd records are guards -- and their references."""

    def __init__(self, cuda, n):
        self.n, self.n_dev = n, 2 * n
        host = np.full(self.n_dev * CSZ + GUARD, FILL, dtype=np.uint8)
        for c in range(n):
            host[2 * c * CSZ:(2 * c + 1) * CSZ] = 0
        self.t = torch.from_numpy(host).to(cuda)
        self.ref = [RefConn() for _ in range(n)]
        self.units = [[] for _ in range(n)]

    def view(self, c):
        """Connection c's carry and the guard record behind it (what check_carry takes)."""
        return self.t[2 * c * CSZ:(2 * c + 2) * CSZ]

    def check(self):
        raw = self.t.cpu().numpy().tobytes()
        out = []
        for c in range(self.n):
            rec = raw[2 * c * CSZ:(2 * c + 1) * CSZ]
            got = np.frombuffer(rec, dtype=_lib.MSG_CARRY)[0]
            for k in _lib.MSG_CARRY.names:
                assert int(got[k]) == self.ref[c].carry[k], (c, k, int(got[k]), self.ref[c].carry[k])
            assert raw[(2 * c + 1) * CSZ:(2 * c + 2) * CSZ] == fill * CSZ, ("the guard behind carry", c)
            out.append(rec)
        assert raw[self.n_dev * CSZ:] == fill * GUARD
        return out


class Multi:
    """One call: reads is a list of dicts -- wire, conn, optionally cap, msg_cap,
    dst_cap, ctl_cap, misalign (added to wire_off), desc (descriptor fields
    overridden last) and expect (DECLINED / INVALID: what both results must say,
    nothing else written)."""

    def __init__(self, cuda, conns, reads, max_len=None):
        self.conns, self.reads, self.n = conns, reads, len(reads)
        self.max_len = max_len if max_len is not None else max(1, max(len(r["wire"]) for r in reads))
        off = 0

        def take(sz, a):
            nonlocal off
            o = align(off, a)
            off = o + sz + GUARD
            return o

        fb = eb = 0
        for r in reads:
            w = r["wire"] = bytes(r["wire"])
            n = len(w)
            r.setdefault("cap", n // 6 + 16)
            r.setdefault("msg_cap", r["cap"])
            r.setdefault("dst_cap", n + 16)
            r.setdefault("ctl_cap", n + 16)
            r["at"] = dict(wire=take(max(n, 16), 256), dst=take(r["dst_cap"], 16), ctl=take(r["ctl_cap"], 1))
            r["fb"], r["eb"] = fb, eb
            fb += r["cap"] + FRAME_GUARD
            eb += r["msg_cap"] + ENTRY_GUARD
        self.sec = {}
        for k, sz in (("frames", fb * FSZ), ("msgs", eb * ESZ), ("res", self.n * DSZ), ("mres", self.n * RSZ),
                      ("reads", self.n * _lib.MSG_READ.itemsize)):
            self.sec[k] = (take(sz, 256), sz)
        host = np.full(align(off, 256), FILL, dtype=np.uint8)
        desc = np.zeros(self.n, dtype=_lib.MSG_READ)
        for i, r in enumerate(reads):
            o, n = r["at"]["wire"], len(r["wire"])
            host[o:o + n] = np.frombuffer(r["wire"], dtype=np.uint8)
            desc[i] = (o, r["at"]["dst"], r["at"]["ctl"], n, 2 * r["conn"], r["dst_cap"], r["ctl_cap"], r["fb"],
                       r["cap"], r["eb"], r["msg_cap"], 0)
            if r.get("misalign"):
                desc[i]["wire_off"] = o + r["misalign"]
            for k, v in r.get("desc", {}).items():
                desc[i][k] = v
        o, sz = self.sec["reads"]
        host[o:o + sz] = desc.view(np.uint8)
        self.host_in = torch.from_numpy(host)
        self.arena = self.host_in.to(cuda)

    def t(self, k):
        o, sz = self.sec[k]
        return self.arena[o:o + sz + GUARD]

    def launch(self, ctx):
        rc = gpu.decode_messages_multi(ctx, self.arena, self.t("reads"), self.n, self.max_len, self.t("frames"),
                                       self.t("msgs"), self.arena, self.arena, self.t("res"), self.t("mres"),
                                       self.conns.t, self.conns.n_dev)
        assert rc == 0, rc

    def expect(self):
        """The references advanced by this call, in read order."""
        self.outs = []
        for r in self.reads:
            if r.get("expect"):
                self.outs.append(None)
                continue
            out = self.conns.ref[r["conn"]].call(r["wire"], r["cap"], r["msg_cap"], r["dst_cap"], r["ctl_cap"])
            self.conns.units[r["conn"]] += out["units"]
            self.outs.append(out)
        return self.outs

    def region(self, got, r, k):
        """Read r's region k with its guard, from the fetched arena."""
        if k in ("wire", "dst", "ctl"):
            sz = {"wire": max(len(r["wire"]), 16), "dst": r["dst_cap"], "ctl": r["ctl_cap"]}[k]
            o = r["at"][k]
            return got[o:o + sz + GUARD].tobytes()
        if k == "frames":
            o = self.sec["frames"][0] + r["fb"] * FSZ
            return got[o:o + (r["cap"] + FRAME_GUARD) * FSZ].tobytes()
        o = self.sec["msgs"][0] + r["eb"] * ESZ
        return got[o:o + (r["msg_cap"] + ENTRY_GUARD) * ESZ].tobytes()

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
            assert self.region(got, r, "dst") == out["dst"] + fill * (r["dst_cap"] + GUARD - len(out["dst"])), ("dst", i)
            assert self.region(got, r, "ctl") == out["ctl"] + fill * (r["ctl_cap"] + GUARD - len(out["ctl"])), ("ctl", i)
            ne = min(len(out["entries"]), r["msg_cap"])
            reg = self.region(got, r, "msgs")
            em = np.frombuffer(reg[:ne * ESZ], dtype=_lib.MSG_INFO)
            for j in range(ne):
                for k in _lib.MSG_INFO.names:
                    assert int(em[j][k]) == out["entries"][j][k], (i, j, k, int(em[j][k]), out["entries"][j][k])
            assert reg[ne * ESZ:] == fill * (len(reg) - ne * ESZ), ("entries past the count", i)
            want, recs = ref_decode_result(r["wire"], r["cap"])
            assert want["n_frames"] == out["n_frames"]
            for k in _lib.DECODE_RESULT.names:
                assert int(res[i][k]) == want[k], (i, k, int(res[i][k]), want[k])
            reg = self.region(got, r, "frames")
            assert reg[:len(recs)] == recs, ("frame records", i)
            assert reg[len(recs):] == fill * (len(reg) - len(recs)), ("frames past the count", i)
        return mres


def run(ctx, cuda, conns, reads, max_len=None):
    """One call, checked in full: returns (the references' outputs, the call, the carries' bytes)."""
    m = Multi(cuda, conns, reads, max_len)
    outs = m.expect()
    m.launch(ctx)
    m.check()
    return outs, m, conns.check()


def key(rng):
    return rng.getrandbits(32)


# ------------------------------------------------------------------ 1. one read = the carry call
@pytest.mark.parametrize("max_len", [SMALL, FULL], ids=["small", "full"])
@pytest.mark.parametrize("seed", range(40))
def test_one_read_equals_the_carry_call(ctx, cuda, seed, max_len):
    wire, _, _ = random_stream(seed)
    conns = Conns(cuda, 1)
    outs, m, carries = run(ctx, cuda, conns, [dict(wire=wire, conn=0)], max_len)
    assert conns.units[0] == whole(wire)[0] and outs[0]["res"]["status"] == 0
    r = m.reads[0]
    c = cc.Call(cuda, wire, cap=r["cap"], msg_cap=r["msg_cap"], dst_cap=r["dst_cap"], ctl_cap=r["ctl_cap"])
    carry = new_carry(cuda)
    c.launch(ctx, carry, with_stream=False)
    single = c.arena.cpu().numpy()

    def of_call(k, extra=GUARD):
        o, sz = c.at[k]
        return single[o:o + sz + extra].tobytes()

    assert m.region(m.got, r, "dst") == of_call("dst")
    assert m.region(m.got, r, "ctl") == of_call("ctl")
    assert m.region(m.got, r, "msgs")[:r["msg_cap"] * ESZ + GUARD] == of_call("msgs")
    assert m.region(m.got, r, "frames")[:r["cap"] * FSZ + GUARD] == of_call("frames")
    assert m.got[m.sec["mres"][0]:][:RSZ + GUARD].tobytes() == of_call("mres")
    mine, theirs = m.got[m.sec["res"][0]:][:DSZ + GUARD].tobytes(), of_call("res")
    cut = _lib.DECODE_RESULT.fields["n_survivors"][1]
    assert cut == DSZ - 4 and mine[:cut] == theirs[:cut] and mine[DSZ:] == theirs[DSZ:]
    assert carries[0] == carry.cpu().numpy().tobytes()[:CSZ]


# ------------------------------------------------------------------ 2. every cut at once
@pytest.mark.parametrize("max_len", [SMALL, FULL], ids=["small", "full"])
def test_every_cut_at_once(ctx, cuda, max_len):
    stream = twelve_frames()
    L = len(stream)
    units, status, _ = whole(stream)
    assert status == 0
    conns = Conns(cuda, L + 1)
    outs, _, _ = run(ctx, cuda, conns, [dict(wire=stream[:c], conn=c) for c in range(L + 1)], max_len)
    resume = [o["res"]["resume_off"] for o in outs]
    outs, _, _ = run(ctx, cuda, conns, [dict(wire=stream[resume[c]:], conn=c) for c in range(L + 1)], max_len)
    continued = sum(1 for o in outs for e in o["entries"] if e["flags"] & cc.CONTINUED)
    assert continued > 40
    for c in range(L + 1):
        assert conns.units[c] == units, c
        assert conns.ref[c].carry["wire_bytes"] == L and outs[c]["res"]["status"] == 0


# ------------------------------------------------------------------ 3. random connections
def test_random_connections_advance_together(ctx, cuda):
    seeds = list(range(40))
    streams = [random_cuts(s) for s in seeds]
    conns = Conns(cuda, len(seeds))
    pos, rounds = [0] * len(seeds), max(len(cuts) for _, cuts in streams) + 1
    calls, continued = [0] * len(seeds), [0] * len(seeds)
    for k in range(rounds):
        reads = []
        for c, (wire, cuts) in enumerate(streams):
            ends = cuts + [len(wire)]
            reads.append(dict(wire=wire[pos[c]:ends[k]] if k < len(ends) else b"", conn=c))
        outs, _, _ = run(ctx, cuda, conns, reads)
        for c, out in enumerate(outs):
            pos[c] += out["res"]["resume_off"]
            if k <= len(streams[c][1]):
                calls[c] += 1
                continued[c] += sum(1 for e in out["entries"] if e["flags"] & cc.CONTINUED)
                assert out["res"]["status"] == 0
    for c, (wire, _) in enumerate(streams):
        assert calls[c] >= 2 and continued[c] >= 1    # the input condition (test_msg_carry_cpu.py)
        assert conns.units[c] == whole(wire)[0], c
        assert conns.ref[c].carry["wire_bytes"] == len(wire) == pos[c]
        assert conns.ref[c].carry["n_msgs"] == len(conns.units[c])


# ------------------------------------------------------------------ 4. gather seams
def test_gather_seams(ctx, cuda):
    rng = random.Random(4)
    wires = []
    for start in range(16):                           # payload start of the first fragment, mod 16
        for first in range(34):
            pad = (start - 12) % 16                   # a PING's 6 + pad bytes, then the 6-byte header
            body = cc.random_text(rng, first + 40) if first % 2 else cc.payload(rng, first + 40)
            op = TEXT if first % 2 else BIN
            w = frame(PING, cc.payload(rng, pad), key=key(rng)) + frame(op, body[:first], fin=0, key=key(rng))
            assert len(w) % 16 == (start + first) % 16 and (len(w) - first) % 16 == start
            wires.append(w + frame(CONT, body[first:], fin=1, key=key(rng)))
    # twenty 1-byte fragments with empty ones between: a 16-B chunk spans more than three frames
    text = cc.random_text(rng, 20)
    w = frame(TEXT, b"", fin=0, key=key(rng))
    for j in range(20):
        w += frame(CONT, text[j:j + 1], fin=0, key=key(rng))
        if j % 3 == 0:
            w += frame(CONT, b"", fin=0, key=key(rng))
    wires.append(w + frame(CONT, b"", fin=1, key=key(rng)))
    # fragments that end exactly at a chunk's end, and one message after them
    wires.append(frame(BIN, cc.payload(rng, 16), fin=0, key=key(rng)) + frame(CONT, cc.payload(rng, 32), fin=0, key=key(rng)) +
                 frame(CONT, cc.payload(rng, 5), fin=1, key=key(rng)) + frame(TEXT, cc.random_text(rng, 27), key=key(rng)))
    conns = Conns(cuda, len(wires))
    outs, _, _ = run(ctx, cuda, conns, [dict(wire=w, conn=c) for c, w in enumerate(wires)])
    for c, w in enumerate(wires):
        assert conns.units[c] == whole(w)[0] and outs[c]["res"]["status"] == 0, c
    assert conns.units[-2][0][:3] == (TEXT, text, 1) and conns.units[-2][0][3] > 25


# ------------------------------------------------------------------ 5. UTF-8 across calls
def test_utf8_across_calls(ctx, cuda):
    rng = random.Random(5)
    pairs, want = [], []                              # (first read, second read), the units after both
    for seq in cc.VALID + cc.ILL_FORMED:
        for cut in range(1, len(seq)):
            pairs.append((frame(TEXT, b"ab" + seq[:cut], fin=0, key=key(rng)),
                          frame(CONT, seq[cut:] + b"cd", fin=1, key=key(rng))))
            want.append([(TEXT, b"ab" + seq + b"cd", int(seq in cc.VALID), 2)])
    assert sorted({len(s) for s in cc.VALID}) == [2, 3, 4]
    # an invalid byte as the last byte of a part: flagged at the byte after it, so one call later
    late = len(pairs)
    pairs.append((frame(TEXT, b"ab\xc0", fin=0, key=key(rng)), frame(CONT, b"cd", fin=0, key=key(rng))))
    want.append([])
    # the tail does not leak into the next message
    leak = len(pairs)
    pairs.append((frame(TEXT, b"ab", fin=0, key=key(rng)),
                  frame(CONT, b"\xe2\x82", fin=1, key=key(rng)) + frame(TEXT, b"\xac", key=key(rng)) +
                  frame(TEXT, b"\xe2", fin=0, key=key(rng))))
    want.append([(TEXT, b"ab\xe2\x82", 0, 2), (TEXT, b"\xac", 0, 1)])
    # a BIN message carries no tail
    binary = len(pairs)
    pairs.append((frame(BIN, b"\xff\xe2", fin=0, key=key(rng)), frame(CONT, b"\x82", fin=0, key=key(rng))))
    want.append([])
    conns = Conns(cuda, len(pairs))
    first, _, _ = run(ctx, cuda, conns, [dict(wire=p[0], conn=c) for c, p in enumerate(pairs)])
    second, _, _ = run(ctx, cuda, conns, [dict(wire=p[1], conn=c) for c, p in enumerate(pairs)])
    for c in range(len(pairs)):
        assert conns.units[c] == want[c], c
    assert (first[late]["carry"]["utf8_bad"], second[late]["carry"]["utf8_bad"]) == (0, 1)
    assert first[late]["carry"]["utf8_tail"] == cc.tail_word(b"ab\xc0")
    assert second[leak]["carry"]["utf8_tail"] == cc.tail_word(b"\xe2") and second[leak]["carry"]["utf8_bad"] == 0
    for out in (first[binary], second[binary]):
        assert (out["carry"]["utf8_tail"], out["carry"]["utf8_bad"], out["carry"]["open_opcode"]) == (0, 0, BIN)


# ------------------------------------------------------------------ 6. isolation
def test_errors_stay_on_their_connection(ctx, cuda):
    rng = random.Random(6)
    good = [random_cuts(s) for s in range(16)]
    opener = frame(TEXT, b"open", fin=0, key=key(rng))
    ok_msg = frame(BIN, b"fine", key=key(rng))
    too_large = bytes([0x82, 0xFF]) + struct.pack(">Q", (1 << 32) + 1) + struct.pack("<I", key(rng))
    # (first read, second read, status, err_frame of the second read)
    seq = _lib.FWS_ERR_SEQUENCE
    ctlf = _lib.FWS_ERR_CONTROL_FRAME
    bad = [
        (ok_msg, frame(CONT, b"stray", key=key(rng)) + ok_msg, seq, 0),
        (ok_msg, ok_msg + frame(CONT, b"stray", key=key(rng)) + ok_msg, seq, 1),
        (opener, frame(TEXT, b"new", key=key(rng)) + ok_msg, seq, 0),
        (opener, frame(CONT, b"!", fin=0, key=key(rng)) + frame(BIN, b"new", key=key(rng)), seq, 1),
        (opener, frame(PING, b"x", fin=0, key=key(rng)) + frame(CONT, b"", fin=1, key=key(rng)), ctlf, 0),
        (ok_msg, ok_msg + frame(PONG, b"x", fin=0, key=key(rng)) + ok_msg, ctlf, 1),
        (opener, frame(PING, cc.payload(rng, 126), key=key(rng)) + ok_msg, ctlf, 0),
        (ok_msg, ok_msg + frame(PING, cc.payload(rng, 200), key=key(rng)) + ok_msg, ctlf, 1),
        (opener, frame(CONT, b"a", fin=0, key=key(rng)) + frame(CONT, b"b", fin=0, key=key(rng), rsv=4) + ok_msg,
         _lib.FWS_ERR_RSV, NONE),
        (ok_msg, ok_msg + bytes([0x83, 0x80]) + struct.pack("<I", key(rng)) + ok_msg, _lib.FWS_ERR_OPCODE, NONE),
        (ok_msg, ok_msg + frame(BIN, b"plain", masked=False) + ok_msg, _lib.FWS_ERR_NOT_MASKED, NONE),
        (opener, frame(PING, b"p", key=key(rng)) + too_large, _lib.FWS_ERR_TOO_LARGE, NONE),
    ]
    n = len(good) + len(bad)
    conns = Conns(cuda, n)
    # the erring connections between the good ones
    order = list(range(n))
    random.Random(66).shuffle(order)
    wires1 = [w[:cuts[0]] for w, cuts in good] + [b[0] for b in bad]
    outs1, _, _ = run(ctx, cuda, conns, [dict(wire=wires1[c], conn=c) for c in order])
    by_conn = {order[i]: o for i, o in enumerate(outs1)}
    wires2 = [w[by_conn[c]["res"]["resume_off"]:] for c, (w, _) in enumerate(good)] + [b[1] for b in bad]
    before = [dict(r.carry) for r in conns.ref]
    outs2, _, _ = run(ctx, cuda, conns, [dict(wire=wires2[c], conn=c) for c in order])
    by_conn = {order[i]: o for i, o in enumerate(outs2)}
    for c, (w, _) in enumerate(good):
        assert conns.units[c] == whole(w)[0] and by_conn[c]["res"]["status"] == 0, c
    for j, (_, second, status, err_frame) in enumerate(bad):
        c, out = len(good) + j, by_conn[len(good) + j]
        assert (out["res"]["status"], out["res"]["err_frame"]) == (status, err_frame), j
        if err_frame == 0:                            # the state before frame 0: nothing moved
            for k in ("open_opcode", "open_frames", "open_bytes", "utf8_tail", "utf8_bad", "wire_bytes", "n_msgs"):
                assert out["carry"][k] == before[c][k], (j, k)
    assert by_conn[len(good) + 3]["carry"]["open_bytes"] == 5 and by_conn[len(good) + 3]["carry"]["open_frames"] == 2


# ------------------------------------------------------------------ 7. capacities
def test_capacities(ctx, cuda):
    rng = random.Random(72)
    head, tail = cc.capacity_stream(rng)
    units, status, _ = whole(head + tail)
    assert status == 0
    conns = Conns(cuda, 8)
    run(ctx, cuda, conns, [dict(wire=head, conn=c) for c in range(8)])
    probe = RefConn()
    probe.carry, probe.body = dict(conns.ref[0].carry), conns.ref[0].body
    full = probe.call(tail)["res"]
    exact = dict(dst_cap=full["data_bytes"], ctl_cap=full["ctl_bytes"], msg_cap=full["n_msgs"])
    short = {1: dict(dst_cap=exact["dst_cap"] - 1), 3: dict(ctl_cap=exact["ctl_cap"] - 1),
             5: dict(msg_cap=exact["msg_cap"] - 1), 7: dict(cap=3)}
    before = conns.check()
    outs, _, after = run(ctx, cuda, conns, [dict(wire=tail, conn=c, **short.get(c, {})) for c in range(8)])
    for c in (1, 3, 5):
        r = outs[c]["res"]
        assert r["status"] == _lib.FWS_ERR_CAPACITY and r["resume_off"] == 0
        assert after[c] == before[c], "the carry moved"
        assert (outs[c]["dst"], outs[c]["ctl"]) == (b"", b"")     # (Multi.check: the regions hold only fill)
        for k in ("n_msgs", "data_bytes", "ctl_bytes"):
            assert r[k] == full[k]
    for c in (0, 2, 4, 6):
        assert outs[c]["res"]["status"] == 0 and conns.units[c] == units
    assert outs[7]["res"]["status"] == _lib.FWS_ERR_CAPACITY and outs[7]["res"]["resume_off"] > 0
    # retried with exact capacities; the read short on frames continues from resume_off
    pos, calls = outs[7]["res"]["resume_off"], 1
    first = True
    while pos < len(tail) or first:
        reads = [dict(wire=tail if first and c in (1, 3, 5) else b"", conn=c, **(exact if c in (1, 3, 5) else {}))
                 for c in range(7)]
        reads.append(dict(wire=tail[pos:], conn=7, cap=3))
        outs, _, _ = run(ctx, cuda, conns, reads)
        if first:
            for c in (1, 3, 5):
                assert outs[c]["res"]["status"] == 0 and outs[c]["res"]["resume_off"] == len(tail)
                assert outs[c]["entries"][0]["flags"] == cc.CONTINUED
        assert outs[7]["res"]["resume_off"] > 0
        pos, calls, first = pos + outs[7]["res"]["resume_off"], calls + 1, False
    assert calls >= 5 and outs[7]["res"]["status"] == 0
    for c in range(8):
        assert conns.units[c] == units, c
        assert conns.ref[c].carry["wire_bytes"] == len(head + tail)


# ------------------------------------------------------------------ 8. limits
def one_frame_of(rng, total, op=BIN):
    """A single frame of exactly `total` wire bytes."""
    hdr = 6 if total - 6 < 126 else (8 if total - 8 <= 65535 else 14)
    body = cc.payload(rng, total - hdr) if op == BIN else cc.random_text(rng, total - hdr)
    w = frame(op, body, key=key(rng))
    assert len(w) == total
    return w


def tiny_frames(rng, n):
    return b"".join(frame(BIN, cc.payload(rng, j % 3), key=key(rng)) for j in range(n))


@pytest.mark.parametrize("max_len", [4096, FULL], ids=["small", "full"])
def test_limits(ctx, cuda, max_len):
    rng = random.Random(8)
    ping = frame(PING, b"are you there", key=key(rng))
    wires = [b"", ping[:1], ping[:5], one_frame_of(rng, max_len, TEXT), tiny_frames(rng, 256)]
    if max_len != FULL:
        wires.append(one_frame_of(rng, max_len // 2))
    accepted = len(wires)
    over, many = one_frame_of(rng, max_len + 16), tiny_frames(rng, 257)
    reads = [dict(wire=w, conn=c) for c, w in enumerate(wires)]
    reads.append(dict(wire=over, conn=accepted, expect=DECLINED))
    reads.append(dict(wire=many, conn=accepted + 1, expect=DECLINED))
    conns = Conns(cuda, accepted + 4)
    reads.append(dict(wire=ping, conn=accepted + 2, expect=INVALID, desc=dict(conn=conns.n_dev)))
    reads.append(dict(wire=b"\0" * 4 + ping, conn=accepted + 3, expect=INVALID, misalign=4))
    m = Multi(cuda, conns, reads, max_len)
    outs = m.expect()
    m.launch(ctx)
    m.check()
    conns.check()
    for c, w in enumerate(wires):
        assert conns.units[c] == whole(w)[0], c
    assert outs[3]["units"][0][2] == 1 and len(outs[4]["units"]) == 256
    assert (outs[1]["res"]["resume_off"], outs[2]["res"]["resume_off"]) == (0, 0)
    # the declined reads through the carry call, with the same carry
    for c, w in ((accepted, over), (accepted + 1, many)):
        call = cc.Call(cuda, w)
        out = conns.ref[c].call(w, call.cap, call.msg_cap, call.dst_cap, call.ctl_cap)
        call.launch(ctx, conns.view(c), with_stream=False)
        call.check(out, with_stream=False)
        check_carry(conns.view(c), out["carry"])
        assert out["units"] == whole(w)[0] and out["res"]["status"] == 0
    conns.check()


# ------------------------------------------------------------------ 9. two calls, no host step between
def test_two_calls_queued_on_one_stream(ctx, cuda):
    n = 24
    conns = Conns(cuda, n)
    firsts, seconds = [], []
    for c in range(n):
        rng = random.Random(900 + c)
        a = cc.good_messages(rng, 1 + c % 5) + frame(TEXT, b"gr\xc3", fin=0, key=key(rng)) + frame(PING, b"mid", key=key(rng))
        b = frame(CONT, b"\xbc\xc3", fin=0, key=key(rng)) + frame(CONT, b"\x9fe", fin=1, key=key(rng))
        b += cc.good_messages(rng, 3 + 7 * (c % 4)) + frame(BIN, b"open", fin=0, key=key(rng))
        firsts.append(dict(wire=a, conn=c))
        seconds.append(dict(wire=b, conn=c))
    calls = [Multi(cuda, conns, firsts), Multi(cuda, conns, seconds)]
    outs = [m.expect() for m in calls]                # frame-aligned reads: the host knows the descriptors
    for c in range(n):
        assert outs[0][c]["res"]["resume_off"] == len(firsts[c]["wire"])
        assert outs[1][c]["entries"][0]["flags"] == cc.CONTINUED
        assert outs[1][c]["units"][0] == (TEXT, "grüße".encode(), 1, 3)
    torch.cuda.synchronize()
    for m in calls:
        m.launch(ctx)
    torch.cuda.synchronize()
    for m in calls:
        m.check()
    conns.check()


# ------------------------------------------------------------------ 10. graph capture
def test_graph_capture_and_replay(cuda):
    """One captured call over fixed-size chunk buffers, replayed three times with
    the buffers refilled: the carries flow through the replays in device memory,
    and the last one delivers each connection's TEXT message that spans all three."""
    n = 8
    chunks = []                                       # per connection: three reads of one length
    for c in range(n):
        rng = random.Random(1000 + c)
        k = 60 + 9 * c
        body = (cc.random_text(rng, k) + "€".encode() + cc.random_text(rng, k - 4) + "\U0001F600".encode() +
                cc.random_text(rng, k))
        parts = [body[:k + 1], body[k + 1:2 * k + 2], body[2 * k + 2:]]
        assert [cc.strict_ok(p) for p in parts] == [0, 0, 0] and cc.strict_ok(body)
        ws = [frame(TEXT if j == 0 else CONT, p, fin=int(j == 2), key=key(rng), len_form=126) +
              frame(PING, cc.payload(rng, 9), key=key(rng)) for j, p in enumerate(parts)]
        assert len(set(map(len, ws))) == 1
        chunks.append(ws)
    conns = Conns(cuda, n)
    c = gpu.Ctx(0)                                    # (no reserve: the call has no workspace)
    try:
        m = Multi(cuda, conns, [dict(wire=chunks[i][0], conn=i, cap=8, msg_cap=8, dst_cap=len(chunks[i][0]),
                                     ctl_cap=len(chunks[i][0])) for i in range(n)])
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            m.launch(c)
        torch.cuda.synchronize()
        conns.check()                                 # captured, not run: the carries are still zero
        for j in range(3):
            host = m.host_in.clone()
            for i, r in enumerate(m.reads):
                w = r["wire"] = chunks[i][j]
                o = r["at"]["wire"]
                host[o:o + len(w)] = torch.from_numpy(np.frombuffer(w, dtype=np.uint8).copy())
            m.arena.copy_(host)
            outs = m.expect()
            g.replay()
            torch.cuda.synchronize()
            m.check()
            conns.check()
        for i in range(n):
            e = outs[i]["entries"][0]
            assert e["flags"] == cc.CONTINUED and outs[i]["units"][0][2:] == (1, 3)
            assert outs[i]["carry"]["prev_open_frames"] + e["n_data_frames"] == 3
    finally:
        torch.cuda.synchronize()
        c.close()


# ------------------------------------------------------------------ 11. MessageMux
def test_message_mux_returns_the_reference_units(ctx, cuda):
    seeds = [3, 5, 8, 11, 17, 21, 29, 33]
    wires = [random_stream(s)[0] for s in seeds]
    # connection 5: a stray continuation between two messages in the middle of its stream
    w5, spans, fragmented = random_stream(seeds[5])
    at = spans[len(spans) // 2][0]
    inside = [a for a, b in fragmented if spans[a][0] < at <= spans[b][0]]
    if inside:                                        # not between the fragments of a message
        at = spans[inside[0]][0]
    wires[5] = w5[:at] + frame(CONT, b"stray", key=7) + w5[at:]
    want = [whole(w) for w in wires]
    assert want[5][1] == _lib.FWS_ERR_SEQUENCE and all(s == 0 for i, (_, s, _) in enumerate(want) if i != 5)
    rng = random.Random(11)
    mux = gpu.MessageMux(ctx, 8, max_read=700, max_frame=2048)
    got, pos, feeds, raised = [[] for _ in wires], [0] * 8, 0, False
    while any(p < len(w) for p, w in zip(pos, wires) if w is not wires[5]) or (not raised):
        reads = {}
        for c, w in enumerate(wires):
            if pos[c] < len(w) and mux.status[c] == 0:
                k = rng.randint(1, 700)
                reads[c] = w[pos[c]:pos[c] + k]
                pos[c] += k
        if mux.status[5] != 0 and not raised:
            with pytest.raises(gpu.FwsError):
                mux.feed({5: b"more", 0: b""})
            raised = True
            assert mux.status[5] == _lib.FWS_ERR_SEQUENCE
        for c, units in mux.feed(reads).items():
            got[c] += units
        feeds += 1
        assert feeds < 100
    for c in range(8):
        assert got[c] == [(op, body, bool(ok)) for op, body, ok, _ in want[c][0]], c
        if c != 5:
            assert mux.status[c] == 0
    carries = np.frombuffer(mux.carries.cpu().numpy().tobytes(), dtype=_lib.MSG_CARRY)
    for c in range(8):
        if c != 5:
            assert int(carries[c]["wire_bytes"]) == len(wires[c]) and int(carries[c]["n_msgs"]) == len(want[c][0])
    assert feeds >= 2 and raised


def test_message_mux_takes_a_declined_read_through_the_carry_call(ctx, cuda):
    rng = random.Random(12)
    many = tiny_frames(rng, 300) + frame(TEXT, b"after", key=key(rng))
    other = random_stream(2)[0][:1500]
    mux = gpu.MessageMux(ctx, 2, max_read=2048, max_frame=2048)
    got = mux.feed({0: many[:2000], 1: other[:700]})
    more = mux.feed({0: many[2000:], 1: other[700:]})
    units = [(op, body, bool(ok)) for op, body, ok, _ in whole(many)[0]]
    assert got[0] + more[0] == units and len(units) == 301
    ref = RefConn()
    want = ref.call(other)["units"]
    assert got[1] + more[1] == [(op, body, bool(ok)) for op, body, ok, _ in want]
