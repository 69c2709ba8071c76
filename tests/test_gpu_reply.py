"""GPU parity of fws_gpu_reply_messages_multi: the reply frames of many
connections -- PONGs, the CLOSE echo, the echo of every data part -- built in one
launch from what a message decode wrote.

Every test decodes with the flow call in Multi's arena (test_gpu_msg_flow.Flow,
checked there against FlowRef) and then replies into a second arena that is
pre-filled with a sentinel and compared whole: each read's region, its frame
records and its fws_tx_result must be ReplyRef's (reply_ref.py), and every other
byte -- the guards on both sides of each region, the rest of a region, the
records past the count, the descriptors -- must be the sentinel or the input.
The fws_tx_conn and fws_reply_state arrays (odd records are guards) are compared
byte for byte as well. All comparisons are exact."""
import random
import struct

import numpy as np
import pytest
import torch

import reply_ref as rr
import test_gpu_msg_carry as cc
import test_gpu_msg_flow as fm
import test_gpu_msg_multi as mm
import txmulti_ref as tr
from flashws_amd import _lib, gpu
from reply_ref import CONTROL, ECHO, ReplyRef, messages, walk_frames
from test_gpu_msg_carry import BIN, CLOSE, CONT, FILL, GUARD, PING, PONG, TEXT, frame, key
from test_gpu_msg_multi import FRAME_GUARD, FSZ, align, fill

pytestmark = pytest.mark.gpu

CAPACITY, DECLINED, INVALID = _lib.FWS_ERR_CAPACITY, _lib.FWS_ERR_DECLINED, _lib.FWS_ERR_INVALID
SMALL, FULL = mm.SMALL, mm.FULL
TSZ, SSZ, RSZ, GSZ = (_lib.TX_CONN.itemsize, _lib.REPLY_STATE.itemsize, _lib.TX_RESULT.itemsize,
                      _lib.REPLY_REGION.itemsize)
BOTH = CONTROL | ECHO
FORMS = pytest.mark.parametrize("max_len", [SMALL, FULL], ids=["small", "full"])


class RConns:
    """The send side of a test's connections: fws_tx_conn and fws_reply_state
    on the device -- record 2c is connection c's, as in the decode's state
    array; the odd records are guards -- and their references."""

    def __init__(self, cuda, n, flags=BOTH):
        self.n, self.n_dev, self.flags = n, 2 * n, flags
        self.tx, self.st = (self._array(cuda, sz) for sz in (TSZ, SSZ))
        self.ref = [ReplyRef(flags) for _ in range(n)]

    def _array(self, cuda, sz):
        host = np.full(self.n_dev * sz + GUARD, FILL, dtype=np.uint8)
        for c in range(self.n):
            host[2 * c * sz:(2 * c + 1) * sz] = 0
        return torch.from_numpy(host).to(cuda)

    def preset(self, c, **state):
        """The host's own write to connection c's reply state."""
        self.ref[c].state = dict(self.ref[c].state, **state)
        rec = np.frombuffer(rr.state_bytes(self.ref[c].state), dtype=np.uint8).copy()
        self.st[2 * c * SSZ:(2 * c + 1) * SSZ] = torch.from_numpy(rec).to(self.st.device)

    def check(self):
        for t, sz, want in ((self.tx, TSZ, lambda r: rr.tx_bytes(r.tx)), (self.st, SSZ, lambda r: rr.state_bytes(r.state))):
            raw = t.cpu().numpy().tobytes()
            for c in range(self.n):
                assert raw[2 * c * sz:(2 * c + 1) * sz] == want(self.ref[c]), (sz, c, self.ref[c].tx, self.ref[c].state)
                assert raw[(2 * c + 1) * sz:(2 * c + 2) * sz] == fill * sz, ("the guard behind the state", sz, c)
            assert raw[self.n_dev * sz:] == fill * GUARD


class Reply:
    """One reply call over a decode call m (its expect() done). opts[i], per
    read: out_cap, frame_cap, out_misalign (added to out_off), mres (fields of
    the read's fws_msg_result overwritten on the device before the call)."""

    def __init__(self, cuda, m, rc, opts=None, flags=None):
        self.m, self.rc, self.n = m, rc, m.n
        self.flags = rc.flags if flags is None else flags
        self.opts = opts = [dict(o) for o in (opts or [{} for _ in range(m.n)])]
        off = 0

        def take(sz, a):
            nonlocal off
            o = align(off + GUARD, a)                 # (a guard in front as well)
            off = o + sz + GUARD
            return o

        fb = 0
        for r, o in zip(m.reads, opts):
            o.setdefault("out_cap", len(r["wire"]) + 10 * (r["msg_cap"] + 1) + 16)
            o.setdefault("frame_cap", r["msg_cap"] + 1)
            o["at"] = take(o["out_cap"], 16)
            o["fb"] = fb
            fb += o["frame_cap"] + FRAME_GUARD
        self.sec = {}
        for k, sz in (("frames", fb * FSZ), ("res", self.n * RSZ), ("regions", self.n * GSZ)):
            self.sec[k] = (take(sz, 256), sz)
        host = np.full(align(off, 256), FILL, dtype=np.uint8)
        desc = np.zeros(self.n, dtype=_lib.REPLY_REGION)
        for i, o in enumerate(opts):
            desc[i] = (o["at"] + o.get("out_misalign", 0), o["out_cap"], o["fb"], o["frame_cap"], 0, 0)
        s, sz = self.sec["regions"]
        host[s:s + sz] = desc.view(np.uint8)
        self.host_in = host
        self.arena = torch.from_numpy(host).to(cuda)
        for i, o in enumerate(opts):                  # a decode output that no decode writes, by hand
            if "mres" in o:
                at = m.sec["mres"][0] + i * mm.RSZ
                rec = np.frombuffer(m.arena[at:at + mm.RSZ].cpu().numpy().tobytes(), dtype=_lib.MSG_RESULT).copy()
                for k, v in o["mres"].items():
                    rec[0][k] = v
                m.arena[at:at + mm.RSZ] = torch.from_numpy(rec.view(np.uint8).copy()).to(cuda)

    def t(self, k):
        o, sz = self.sec[k]
        return self.arena[o:o + sz + GUARD]

    def expect(self):
        """The references advanced by this call; the arena as it must look afterwards."""
        want = self.host_in.copy()
        self.outs = []
        for i, (r, o) in enumerate(zip(self.m.reads, self.opts)):
            out = self.m.outs[i] if self.m.outs[i] is not None else rr.undecoded(r["expect"])
            if "mres" in o:
                out = dict(out, res=dict(out["res"], **o["mres"]))
            got = self.rc.ref[r["conn"]].call(
                out, msg_cap=r["msg_cap"], dst_cap=r["dst_cap"], ctl_cap=r["ctl_cap"], out_cap=o["out_cap"],
                frame_cap=o["frame_cap"], out_off=o["at"] + o.get("out_misalign", 0),
                conn_ok=r.get("desc", {}).get("conn", 0) < self.rc.n_dev)
            self.outs.append(got)
            b = np.frombuffer(got["bytes"], dtype=np.uint8)
            want[o["at"]:o["at"] + len(b)] = b
            rec = got["records"].tobytes()
            at = self.sec["frames"][0] + o["fb"] * FSZ
            want[at:at + len(rec)] = np.frombuffer(rec, dtype=np.uint8)
            res = np.zeros(1, dtype=_lib.TX_RESULT)
            for k, v in got["res"].items():
                res[0][k] = v
            at = self.sec["res"][0] + i * RSZ
            want[at:at + RSZ] = res.view(np.uint8)
        self.want = want
        return self.outs

    def launch(self, ctx, stream=None):
        m = self.m
        rc = gpu.reply_messages_multi(ctx, m.t("reads"), m.n, m.max_len, m.t("msgs"), m.arena, m.arena, m.t("mres"),
                                      self.t("regions"), self.arena, self.t("frames"), self.t("res"), self.rc.tx,
                                      self.rc.st, self.rc.n_dev, self.flags, stream=stream)
        assert rc == 0, rc

    def check(self):
        got = self.got = self.arena.cpu().numpy()
        res = np.frombuffer(got[self.sec["res"][0]:][:self.n * RSZ].tobytes(), dtype=_lib.TX_RESULT)
        for i, (o, out) in enumerate(zip(self.opts, self.outs)):
            for k in _lib.TX_RESULT.names:
                assert int(res[i][k]) == out["res"][k], ("result", i, k, int(res[i][k]), out["res"][k])
            a, n = o["at"], len(out["bytes"])
            assert got[a - GUARD:a].tobytes() == fill * GUARD, ("the guard in front of region", i)
            if got[a:a + n].tobytes() != out["bytes"]:
                bad = next(j for j in range(n) if got[a + j] != out["bytes"][j])
                assert False, ("region", i, "first wrong byte", bad, "of", n, out["res"])
            assert got[a + n:a + o["out_cap"] + GUARD].tobytes() == fill * (o["out_cap"] + GUARD - n), \
                ("behind the frames of region", i)
        diff = np.nonzero(got != self.want)[0]
        assert diff.size == 0, ("the arena differs at", int(diff[0]), self.sec)

    def region(self, i):
        a = self.opts[i]["at"]
        return self.got[a:a + self.outs[i]["res"]["out_len"]].tobytes()


def reply(ctx, cuda, m, rc, opts=None, flags=None):
    rp = Reply(cuda, m, rc, opts, flags)
    rp.expect()
    rp.launch(ctx)
    torch.cuda.synchronize()
    rp.check()
    rc.check()
    return rp


def step(ctx, cuda, conns, rc, reads, max_len=None, opts=None):
    """decode + reply, both checked in full: (the decode's outputs, the reply call)."""
    outs, m, _ = fm.run(ctx, cuda, conns, reads, max_len)
    return outs, reply(ctx, cuda, m, rc, opts)


def binmsg(rng, n, op=BIN):
    return frame(op, cc.payload(rng, n), key=key(rng))


# ------------------------------------------------------------------ 1. header forms and tails
@pytest.mark.parametrize("flags", [0, CONTROL, ECHO, BOTH], ids=["none", "control", "echo", "both"])
def test_header_forms_and_tails(ctx, cuda, flags):
    rng = random.Random(1)
    sizes = (0, 1, 15, 16, 17, 125, 126, 65535, 65536)
    wires = [binmsg(rng, n) for n in sizes]
    wires += [frame(PING, cc.payload(rng, n), key=key(rng)) for n in (0, 1, 125)]
    wires += [frame(PONG, b"pong", key=key(rng))]
    closes = [b"", b"\x03", struct.pack(">H", 1000), struct.pack(">H", 4999) + cc.payload(rng, 123)]
    wires += [frame(CLOSE, p, key=key(rng)) for p in closes]
    n = len(wires)
    conns, rc = fm.Conns(cuda, n), RConns(cuda, n, flags)
    _, rp = step(ctx, cuda, conns, rc, [dict(wire=w, conn=c) for c, w in enumerate(wires)])
    frames = [o["res"]["n_frames"] for o in rp.outs]
    echo, ctl = int(bool(flags & ECHO)), int(bool(flags & CONTROL))
    assert frames == [echo] * 9 + [ctl] * 3 + [0] + [ctl] * 4
    if flags & ECHO:
        assert [o["records"][0]["hdr_len"] for o in rp.outs[:9]] == [2, 2, 2, 2, 2, 2, 4, 4, 10]
    codes = [r.state["close_code"] for r in rc.ref[13:]]
    assert codes == ([1005, 1005, 1000, 4999] if ctl else [0] * 4)


# ------------------------------------------------------------------ 2. irregular seams
def seam_reads(rng):
    """Frames of 3 to 19 bytes with 2-byte PONGs between them, so that
    several share a 16-B chunk and no source is aligned; a PING between two
    fragments of one message."""
    a = b""
    for j, n in enumerate((1, 2, 3, 5, 13, 17)):
        a += binmsg(rng, n, TEXT if j % 2 else BIN)
        for _ in range((2, 1, 0, 0, 0, 0)[j]):        # two PINGs in a row, then one more
            a += frame(PING, b"", key=key(rng))
    body = cc.payload(rng, 41)
    b = (frame(BIN, body[:7], fin=0, key=key(rng)) + frame(PING, b"between", key=key(rng)) +
         frame(CONT, body[7:], fin=1, key=key(rng)))
    return a, b


@FORMS
def test_irregular_seams(ctx, cuda, max_len):
    a, b = seam_reads(random.Random(2))
    conns, rc = fm.Conns(cuda, 2), RConns(cuda, 2)
    _, rp = step(ctx, cuda, conns, rc, [dict(wire=a, conn=0), dict(wire=b, conn=1)], max_len)
    fa = rp.outs[0]["frames"]
    assert [len(p) for _, _, p in fa] == [1, 0, 0, 2, 0, 3, 5, 13, 17] and fa[1][0] == fa[2][0] == PONG
    # three 2-byte PONGs and a 1-byte message in the first chunk
    assert rp.outs[0]["records"][4]["hdr_off"] < 16 and rp.outs[0]["res"]["out_len"] == 41 + 12 + 6
    assert [(op, fin, len(p)) for op, fin, p in rp.outs[1]["frames"]] == [(PONG, 1, 7), (BIN, 1, 41)]


# ------------------------------------------------------------------ 3. parts
def test_parts_become_continuations(ctx, cuda):
    rng = random.Random(3)
    body = cc.payload(rng, 300)
    whole = frame(TEXT, body[:200], fin=0, key=key(rng)) + frame(CONT, body[200:], fin=1, key=key(rng))
    lead = frame(BIN, body[:150], key=key(rng))
    after = binmsg(rng, 9)
    streams = [whole, whole, lead + after, frame(BIN, body[:40], fin=0, key=key(rng))]
    #         inside the first fragment; its header alone (an open part of 0 bytes); inside a FIN frame; a whole
    #         fragment, then nothing
    cuts = [61, 8, 100, len(streams[3])]
    conns, rc = fm.Conns(cuda, 4), RConns(cuda, 4)
    _, first = step(ctx, cuda, conns, rc, [dict(wire=s[:c], conn=i) for i, (s, c) in enumerate(zip(streams, cuts))])
    assert [o["frames"] for o in first.outs] == [[(TEXT, 0, body[:53])], [], [(BIN, 0, body[:92])],
                                                 [(BIN, 0, body[:40])]]
    assert [r.tx["last_msg_not_fin"] for r in rc.ref] == [1, 0, 1, 1]
    outs, second = step(ctx, cuda, conns, rc, [dict(wire=s[c:], conn=i) for i, (s, c) in enumerate(zip(streams, cuts))])
    assert all(o["entries"][0]["flags"] == _lib.FWS_MSG_CONTINUED for o in outs[:3]) and not outs[3]["entries"]
    assert second.outs[0]["frames"] == [(0, 1, body[53:])]                       # a continuation with FIN
    assert second.outs[1]["frames"] == [(TEXT, 1, body)]                         # nothing was echoed: the opcode
    assert [(op, fin) for op, fin, _ in second.outs[2]["frames"]] == [(0, 1), (BIN, 1)]   # the lead completes
    assert second.outs[3]["frames"] == [] and second.outs[3]["res"]["last_msg_not_fin"] == 1
    assert [r.tx["last_msg_not_fin"] for r in rc.ref] == [0, 0, 0, 1]
    for c in range(3):
        assert messages(walk_frames(rc.ref[c].wire))[0] == [(u[0], u[1]) for u in conns.units[c]]


# ------------------------------------------------------------------ 4. every cut
def closing_stream():
    """A TEXT message in three fragments with multi-byte sequences and a PING
    inside it, a BIN message, a CLOSE, one more message: about 300 bytes."""
    rng = random.Random(4)
    text = cc.random_text(rng, 150)
    f = [frame(TEXT, text[:31], fin=0, key=key(rng)), frame(CONT, text[31:127], fin=0, key=key(rng), len_form=126),
         frame(PING, b"are you there", key=key(rng)), frame(CONT, text[127:], fin=1, key=key(rng)),
         frame(BIN, cc.payload(rng, 60), key=key(rng)), frame(CLOSE, struct.pack(">H", 1001) + b"going", key=key(rng)),
         frame(TEXT, b"too late", key=key(rng))]
    return b"".join(f)


@pytest.mark.parametrize("flags", [BOTH, ECHO], ids=["both", "echo"])
def test_every_cut_at_once(ctx, cuda, flags):
    stream = closing_stream()
    L = len(stream)
    assert 280 <= L <= 330
    uncut = ReplyRef(flags)
    uncut.call(fm.FlowRef().call(stream))
    units, still_open = messages(walk_frames(uncut.wire))
    assert still_open is None and len(units) == (4 if flags & CONTROL else 3)
    n = L + 1
    conns, rc = fm.Conns(cuda, n), RConns(cuda, n, flags)
    pos, rounds, silent = [0] * n, 0, 0
    for ends in ([c for c in range(n)], [L] * n):
        outs, rp = step(ctx, cuda, conns, rc, [dict(wire=stream[pos[c]:ends[c]], conn=c) for c in range(n)])
        for c, out in enumerate(outs):
            pos[c] += out["res"]["resume_off"]
        silent += sum(1 for o, r in zip(rp.outs, rp.m.reads) if rc.ref[r["conn"]].state["close_sent"] and
                      not o["res"]["n_frames"] and len(r["wire"]))
        rounds += 1
    assert rounds == 2 and pos == [L] * n
    if flags & CONTROL:
        assert silent > 5                             # cuts behind the CLOSE: the second call writes nothing
    for c in range(n):
        got, still_open = messages(walk_frames(rc.ref[c].wire))   # (nothing follows the CLOSE: asserted there)
        assert got == units and still_open is None, c
        assert rc.ref[c].state == uncut.state


# ------------------------------------------------------------------ 5. after the CLOSE
def test_nothing_follows_the_close(ctx, cuda):
    rng = random.Random(5)
    closing = binmsg(rng, 20) + frame(CLOSE, struct.pack(">H", 1000), key=key(rng)) + binmsg(rng, 30) + \
        frame(PING, b"late", key=key(rng)) + frame(CLOSE, struct.pack(">H", 1002), key=key(rng))
    conns, rc = fm.Conns(cuda, 3), RConns(cuda, 3)
    rc.preset(1, close_sent=1)                        # the host sent a CLOSE itself
    rc.check()
    _, rp = step(ctx, cuda, conns, rc, [dict(wire=closing, conn=0), dict(wire=closing, conn=1),
                                        dict(wire=binmsg(rng, 5), conn=2)])
    assert [(op, fin, len(p)) for op, fin, p in rp.outs[0]["frames"]] == [(BIN, 1, 20), (CLOSE, 1, 2)]
    assert rp.outs[1]["res"] == dict(tr.refusal(0)) and rc.ref[1].state == dict(close_sent=1, close_code=0, reserved=0)
    assert rc.ref[0].state["close_code"] == 1000 and rp.outs[2]["res"]["n_frames"] == 1
    _, rp = step(ctx, cuda, conns, rc, [dict(wire=binmsg(rng, 8) + frame(PING, b"x", key=key(rng)), conn=c)
                                        for c in range(3)])
    assert [o["res"]["n_frames"] for o in rp.outs] == [0, 0, 2]
    assert rc.ref[0].tx["frames"] == 2 and rc.ref[1].tx["frames"] == 0


# ------------------------------------------------------------------ 6. the table's limit
@FORMS
def test_257_entries_and_258_frames(ctx, cuda, max_len):
    rng = random.Random(6)
    opener = frame(BIN, cc.payload(rng, 30), key=key(rng))
    ones = [frame(TEXT if j % 3 else BIN, bytes([65 + j % 26]), key=key(rng)) for j in range(256)]
    part = frame(BIN, b"z", fin=0, key=key(rng))
    conns, rc = fm.Conns(cuda, 3), RConns(cuda, 3)
    step(ctx, cuda, conns, rc, [dict(wire=opener[:16], conn=c) for c in range(3)], max_len)
    reads = [dict(wire=opener[16:] + b"".join(ones), conn=0),              # 257 entries
             dict(wire=opener[16:] + b"".join(ones[:255]) + part, conn=1),  # 256 and an open part
             dict(wire=opener[16:] + b"".join(ones), conn=2)]               # 257 and an open part, by hand
    # (a decode stops at 256 headers, so it never reports 257 entries and an open part: the last message of
    # connection 2 is declared open once more, which makes the 258 items the table is sized for)
    by_hand = dict(open_opcode=BIN, open_len=1, open_off=0)
    outs, rp = step(ctx, cuda, conns, rc, reads, max_len, opts=[{}, {}, dict(mres=by_hand)])
    assert [len(o["entries"]) for o in outs] == [257, 256, 257] and outs[1]["res"]["open_len"] == 1
    assert [o["res"]["n_frames"] for o in rp.outs] == [257, 257, 258]
    assert rp.outs[0]["frames"][0][:2] == (0, 1) and rp.outs[2]["frames"][-1][:2] == (BIN, 0)
    assert [r.tx["last_msg_not_fin"] for r in rc.ref] == [0, 1, 1]
    # one entry more is not a decode output
    outs, m, _ = fm.run(ctx, cuda, conns, [dict(wire=b"".join(ones[:4]), conn=0, msg_cap=300)], max_len)
    rp = reply(ctx, cuda, m, rc, opts=[dict(mres=dict(n_msgs=258), out_cap=4096)])
    assert rp.outs[0]["res"] == tr.refusal(INVALID)


# ------------------------------------------------------------------ 7. capacity
def test_capacity_is_refused_whole_and_retried(ctx, cuda):
    rng = random.Random(7)
    wire = binmsg(rng, 200) + frame(PING, b"ping", key=key(rng)) + frame(TEXT, b"part", fin=0, key=key(rng))
    need = 204 + 6 + 6
    conns, rc = fm.Conns(cuda, 2), RConns(cuda, 2)
    _, m, _ = fm.run(ctx, cuda, conns, [dict(wire=wire, conn=0), dict(wire=wire, conn=1)])
    rp = reply(ctx, cuda, m, rc, opts=[dict(out_cap=need - 1), dict(out_cap=need)])
    assert rp.outs[0]["res"] == tr.refusal(CAPACITY, 3, need) and rp.outs[1]["res"]["out_len"] == need
    assert rc.ref[0].tx == rr.new_tx() and rc.ref[1].tx["last_msg_not_fin"] == 1
    m.outs[1] = rr.undecoded(DECLINED)                # (connection 1 is done: its read is not answered twice)
    rp = Reply(cuda, m, rc, opts=[dict(out_cap=need), dict(out_cap=need, mres=dict(status=DECLINED))])
    rp.expect()
    rp.launch(ctx)
    torch.cuda.synchronize()
    rp.check()
    rc.check()
    assert rp.outs[0]["res"]["status"] == 0 and rp.region(0) == rc.ref[1].wire


# ------------------------------------------------------------------ 8. isolation
def test_refused_reads_leave_their_neighbours_alone(ctx, cuda):
    rng = random.Random(8)
    good = binmsg(rng, 50) + frame(PING, b"p", key=key(rng))
    conns, rc = fm.Conns(cuda, 6), RConns(cuda, 6)
    reads = [dict(wire=good, conn=0),
             dict(wire=good, conn=1),                                              # out_off misaligned
             dict(wire=good, conn=2, expect=INVALID, desc=dict(conn=conns.n_dev)),  # conn >= n_conns
             dict(wire=good + bytes(40), conn=3, expect=DECLINED),                 # a declined decode
             dict(wire=good, conn=4, dst_cap=32),                                  # a decode over its dst_cap
             dict(wire=good, conn=5)]
    outs, m, _ = fm.run(ctx, cuda, conns, reads, max_len=len(good))
    assert outs[4]["res"]["status"] == CAPACITY and outs[4]["res"]["data_bytes"] == 50
    rp = reply(ctx, cuda, m, rc, opts=[{}, dict(out_misalign=8), {}, {}, {}, {}])
    assert [o["res"]["status"] for o in rp.outs] == [0, INVALID, INVALID, 0, 0, 0]
    assert [o["res"]["n_frames"] for o in rp.outs] == [2, 0, 0, 0, 0, 2]
    assert rp.region(0) == rp.region(5) and all(rc.ref[c].tx == rr.new_tx() for c in (1, 2, 3, 4))


# ------------------------------------------------------------------ 9. both forms
def test_a_100_kib_message_at_dst_offset_3(ctx, cuda):
    rng = random.Random(9)
    body = np.random.default_rng(9).integers(0, 256, 100 << 10, dtype=np.uint8).tobytes()
    wire = frame(TEXT, b"abc", key=key(rng)) + frame(BIN, body, key=key(rng)) + frame(PING, b"", key=key(rng))
    wire += frame(BIN, cc.payload(rng, (128 << 10) - len(wire) - 8), fin=0, key=key(rng))
    assert len(wire) == 128 << 10
    conns, rc = fm.Conns(cuda, 1), RConns(cuda, 1)
    outs, rp = step(ctx, cuda, conns, rc, [dict(wire=wire, conn=0)], FULL)
    assert outs[0]["entries"][1]["off"] == 3 and outs[0]["entries"][1]["len"] == 100 << 10
    assert [(op, fin) for op, fin, _ in rp.outs[0]["frames"]] == [(TEXT, 1), (BIN, 1), (PONG, 1), (BIN, 0)]


def test_both_forms_write_the_same_bytes(ctx, cuda):
    regions = []
    for max_len in (SMALL, FULL):
        rng = random.Random(10)
        a, b = seam_reads(rng)
        reads = [dict(wire=a, conn=0), dict(wire=b, conn=1), dict(wire=closing_stream(), conn=2),
                 dict(wire=binmsg(rng, 4000) + binmsg(rng, 4001, TEXT), conn=3)]
        conns, rc = fm.Conns(cuda, 4), RConns(cuda, 4)
        _, rp = step(ctx, cuda, conns, rc, reads, max_len)
        regions.append([rp.region(i) for i in range(4)])
    assert regions[0] == regions[1] and all(regions[0])


# ------------------------------------------------------------------ 10. chaining
def three_rounds(n):
    """n connections' streams, each cut in three at its own places."""
    rounds = [[], [], []]
    for c in range(n):
        rng = random.Random(1100 + c)
        s = cc.good_messages(rng, 2 + c % 3) + frame(TEXT, cc.random_text(rng, 80 + 5 * c), key=key(rng))
        s += frame(PING, b"mid", key=key(rng)) + cc.good_messages(rng, 2) + frame(BIN, b"open", fin=0, key=key(rng))
        probe, pos = fm.FlowRef(), 0
        for k, end in enumerate((len(s) // 3 + c % 7, 2 * len(s) // 3 - c % 5, len(s))):
            rounds[k].append(dict(wire=s[pos:end], conn=c))
            pos += probe.call(s[pos:end])["res"]["resume_off"]
    return rounds


def test_three_decodes_and_replies_queued_on_one_stream(ctx, cuda):
    n = 16
    conns, rc = fm.Conns(cuda, n), RConns(cuda, n)
    calls = []
    for reads in three_rounds(n):
        m = fm.Flow(cuda, conns, reads)
        m.expect()
        rp = Reply(cuda, m, rc)
        rp.expect()
        calls.append((m, rp))
    assert any(o["state"]["frame_unread"] for m, _ in calls[:2] for o in m.outs)
    torch.cuda.synchronize()
    for m, rp in calls:                               # six launches, nothing in between
        m.launch(ctx)
        rp.launch(ctx)
    torch.cuda.synchronize()
    for m, rp in calls:
        m.check()
        rp.check()
    conns.check()
    rc.check()
    for c in range(n):
        units, still_open = messages(walk_frames(rc.ref[c].wire))
        assert still_open == (BIN, b"open") and len(units) >= 5


def test_graph_capture_of_decode_and_reply_replayed_on_two_inputs(cuda):
    """decode + reply captured once; the replays' inputs differ in every payload
    byte and in the connections' states, and each equals the eager result."""
    n = 6

    def inputs(seed):
        rng = random.Random(seed)
        return [dict(wire=binmsg(rng, 10 + 30 * c) + frame(PING, cc.payload(rng, c), key=key(rng)) +
                     frame(TEXT, cc.random_text(rng, 50), fin=0, key=key(rng)), conn=c) for c in range(n)]

    c = gpu.Ctx(0)
    try:
        eager = []
        for seed in (21, 22):
            conns, rc = fm.Conns(cuda, n), RConns(cuda, n)
            if seed == 22:                            # the second input finds messages open
                fm.run(c, cuda, conns, [dict(wire=frame(BIN, b"first", fin=0, key=seed), conn=k) for k in range(n)])
                for k in range(n):
                    rc.ref[k].tx["last_msg_not_fin"] = 1
                rc.tx[0:rc.n_dev * TSZ:2 * TSZ] = 1
                rc.check()
                reads = [dict(r, wire=frame(CONT, b"", fin=1, key=seed) + r["wire"]) for r in inputs(seed)]
            else:
                reads = [dict(r, wire=frame(PONG, b"", key=seed) + r["wire"]) for r in inputs(seed)]
            before = (conns.t.clone(), rc.tx.clone(), rc.st.clone())
            m = fm.Flow(cuda, conns, reads)
            m.expect()
            rp = Reply(cuda, m, rc)
            rp.expect()
            clean = (m.arena.clone(), rp.arena.clone())
            m.launch(c)
            rp.launch(c)
            torch.cuda.synchronize()
            m.check()
            rp.check()
            rc.check()
            eager.append(dict(m=m, rp=rp, conns=conns, rc=rc, before=before, clean=clean,
                              after=(m.arena.clone(), rp.arena.clone(), conns.t.clone(), rc.tx.clone(), rc.st.clone())))
        a, b = eager
        assert a["m"].sec == b["m"].sec and a["rp"].sec == b["rp"].sec          # one layout: one graph serves both
        assert [r["at"] for r in a["m"].reads] == [r["at"] for r in b["m"].reads]
        m, rp, conns, rc = a["m"], a["rp"], a["conns"], a["rc"]
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            m.launch(c)
            rp.launch(c)
        torch.cuda.synchronize()
        for e in (a, b, a):
            for t, src in zip((m.arena, rp.arena, conns.t, rc.tx, rc.st), e["clean"] + e["before"]):
                t.copy_(src)
            g.replay()
            torch.cuda.synchronize()
            for t, want in zip((m.arena, rp.arena, conns.t, rc.tx, rc.st), e["after"]):
                assert torch.equal(t, want)
        assert not torch.equal(a["after"][1], b["after"][1])
    finally:
        torch.cuda.synchronize()
        c.close()


# ------------------------------------------------------------------ 11. the carry form's output
def test_the_output_of_decode_messages_multi(ctx, cuda):
    rng = random.Random(12)
    wires = [cc.good_messages(rng, 5) + frame(PING, b"carry", key=key(rng)) + frame(TEXT, b"half", fin=0, key=key(rng)),
             cc.twelve_frames()]
    conns, rc = mm.Conns(cuda, 2), RConns(cuda, 2)
    _, m, _ = mm.run(ctx, cuda, conns, [dict(wire=w, conn=c) for c, w in enumerate(wires)])
    rp = reply(ctx, cuda, m, rc)
    assert rp.outs[0]["frames"][-2:] == [(PONG, 1, b"carry"), (TEXT, 0, b"half")]
    units, still_open = messages(walk_frames(rp.region(1)))
    assert still_open is None and units[-1] == (CLOSE, struct.pack(">H", 1000) + b"bye")
    assert units == [(PONG if u[0] == PING else u[0], u[1]) for u in conns.units[1] if u[0] != PONG]


# ------------------------------------------------------------------ 12. the application's own sends
def test_an_application_send_continues_an_echoed_part(ctx, cuda):
    rng = random.Random(13)
    conns, rc = fm.Conns(cuda, 2), RConns(cuda, 2)
    step(ctx, cuda, conns, rc, [dict(wire=frame(BIN, b"echoed part", fin=0, key=key(rng)), conn=0),
                                dict(wire=frame(BIN, b"whole", key=key(rng)), conn=1)])
    assert [r.tx["last_msg_not_fin"] for r in rc.ref] == [1, 0]
    payload = b"the application's own bytes"
    sends = np.zeros(2, dtype=_lib.TX_SEND)
    for i in range(2):
        sends[i]["src_off"], sends[i]["out_off"], sends[i]["len"], sends[i]["out_cap"] = 0, 64 * i, len(payload), 64
        sends[i]["conn"], sends[i]["frame_type"], sends[i]["last"] = 2 * i, BIN, 1
    src = torch.from_numpy(np.frombuffer(payload, dtype=np.uint8).copy()).to(cuda)
    out = torch.full((128,), FILL, dtype=torch.uint8, device=cuda)
    res = torch.zeros(2 * RSZ, dtype=torch.uint8, device=cuda)
    d_sends = torch.from_numpy(sends.view(np.uint8).copy()).to(cuda)
    assert gpu.encode_messages_multi(ctx, out, src, d_sends, 2, 64, None, res, rc.tx, rc.n_dev) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy().tobytes()
    for i in range(2):
        want = tr.predict(rc.ref[i].tx, payload, BIN, 1, masked=False)
        assert got[64 * i:64 * i + len(want["bytes"])] == want["bytes"] and want["res"]["status"] == 0
        rc.ref[i].tx = want["state"]
    assert got[0] == 0x80 and got[64] == 0x82         # a continuation with FIN; a new BIN message
    rc.check()


# ------------------------------------------------------------------ 13. end to end
def test_sender_to_responder_and_back(ctx, cuda):
    rng = random.Random(14)
    n, max_read = 4, 4096
    sender = gpu.MessageSender(ctx, n, max_send=32 << 10)
    flow = gpu.MessageFlow(ctx, n, max_read=max_read)
    responder = gpu.MessageResponder(flow, BOTH)
    sent = [[(BIN, cc.payload(rng, 700)), (PING, b"alive?"), (TEXT, cc.random_text(rng, 333))],
            [(TEXT, cc.random_text(rng, 10000)), (BIN, b"")],                  # a message over max_read
            [(PING, b""), (BIN, cc.payload(rng, 4096)), (CLOSE, struct.pack(">H", 1000) + b"done"), (BIN, b"late")],
            [(BIN, cc.payload(rng, 1)), (PONG, b"unasked")]]
    wires = [b"" for _ in range(n)]
    for k in range(max(map(len, sent))):
        out = sender.send({c: (s[k][0], s[k][1], True) for c, s in enumerate(sent) if k < len(s)}, max_frame=3000)
        for c, b in out.items():
            wires[c] += b
    replies, units, pos = [b""] * n, [[] for _ in range(n)], [0] * n
    while any(p < len(w) for p, w in zip(pos, wires)):
        reads = {}
        for c, w in enumerate(wires):
            if pos[c] < len(w):
                k = rng.randint(1, max_read)
                reads[c] = w[pos[c]:pos[c] + k]
                pos[c] += k
        got, back = responder.feed(reads)
        assert set(got) == set(back) == set(reads)
        for c in reads:
            units[c] += got[c]
            replies[c] += back[c]
    assert responder.calls == flow.calls
    for c, s in enumerate(sent):
        assert [(op, body) for op, body, _ in units[c]] == s, c
        answered, still_open = messages(walk_frames(replies[c]))
        want = []
        for op, body in s:
            if op != PONG:
                want.append((PONG if op == PING else op, body))
            if op == CLOSE:
                break
        assert answered == want and still_open is None, c
    assert len(walk_frames(replies[1])) > 3           # the 10000-byte message went back in parts
    assert int(gpu.read_reply_state(responder.states, 2)["close_code"]) == 1000
    assert int(gpu.read_tx_conn(responder.conns, 1)["last_msg_not_fin"]) == 0
