"""GPU parity of fws_gpu_decode_messages_carry: a connection's stream decoded
read by read, the open message and its UTF-8 state carried in device memory.

The oracle is a pure-Python walk written here (RefConn): struct for the
headers, XOR for the keys, bytes.decode("utf-8", "strict") for the verdicts,
and rules (A) / (B) of the UTF-8 check (fws_device.h) restated bytewise for
the positional part of the contract (utf8_bad). The invariant: for any way of
cutting a stream into calls, the units delivered are those of the one-call
decode of the whole stream -- same order, opcodes, bytes (the parts joined),
fragment counts, verdicts, control bytes, and the same first error at the
same frame.

Every call checks, against the walk: the wire unchanged, the guard bytes after
every buffer, dev_frames / *dev_result equal to fws_gpu_decode_stream on the
same bytes, every fws_msg_result, fws_msg_info and fws_msg_carry field, dst
and ctl. The file runs under both resolve modes."""
import math
import random
import struct

import numpy as np
import pytest
import torch

from flashws_amd import _lib, gpu
from wsframes import frame

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
GUARD = 64
FILL = 0xA5
TEXT, BIN, CONT, CLOSE, PING, PONG = 1, 2, 0, 8, 9, 10
CONTINUED = _lib.FWS_MSG_CONTINUED
BIG = 1 << 30

RESOLVE_MODES = {"super_tile": 0, "big_st": 1}


@pytest.fixture(params=list(RESOLVE_MODES), autouse=True)
def resolve_mode(request):
    L = _lib.lib()
    old = L.fws_internal_set_resolve_mode(RESOLVE_MODES[request.param])
    yield request.param
    L.fws_internal_set_resolve_mode(old)


# ------------------------------------------------------------------ reference
def ref_parse(wire):
    """ParseFrameHdr over the stream (server side): frames with complete headers, status."""
    frames, pos, n, status = [], 0, len(wire), 0
    while pos < n:
        avail = n - pos
        if avail < 2:
            break
        b0, b1 = wire[pos], wire[pos + 1]
        op = b0 & 15
        if op not in (0, 1, 2, 8, 9, 10):
            status = _lib.FWS_ERR_OPCODE
            break
        if b0 & 0x70:
            status = _lib.FWS_ERR_RSV
            break
        plen, h = b1 & 127, 2
        if plen == 126:
            if avail < 4:
                break
            plen, h = struct.unpack(">H", wire[pos + 2:pos + 4])[0], 4
        elif plen == 127:
            if avail < 10:
                break
            plen, h = struct.unpack(">Q", wire[pos + 2:pos + 10])[0], 10
        if plen > 1 << 32:
            status = _lib.FWS_ERR_TOO_LARGE
            break
        if not b1 & 0x80:
            status = _lib.FWS_ERR_NOT_MASKED
            break
        if avail < h + 4:
            break
        key = wire[pos + h:pos + h + 4]
        h += 4
        frames.append(dict(hdr_off=pos, hdr_len=h, plen=plen, key=key, op=op, fin=b0 >> 7,
                           trunc=pos + h + plen > n))
        pos += h + plen
    return frames, status


def unmask(wire, f):
    po = f["hdr_off"] + f["hdr_len"]
    raw = np.frombuffer(wire[po:po + f["plen"]], dtype=np.uint8)
    k = np.frombuffer(bytes(f["key"]) * (len(raw) // 4 + 1), dtype=np.uint8)[:len(raw)]
    return (raw ^ k).tobytes()


INVALID_BYTES = frozenset((0xC0, 0xC1)) | frozenset(range(0xF5, 0x100))


def utf8_flagged(b, j):
    """Is byte position j of b (zeros past its end) in error: rule (A), a
    continuation exactly where a lead in j-1..j-3 expects one, and rule (B), the
    invalid bytes and the narrowed second bytes, both seen from the byte after."""
    n = len(b)
    x = b[j] if j < n else 0
    p1 = b[j - 1] if 1 <= j <= n else 0
    p2 = b[j - 2] if 2 <= j <= n + 1 else 0
    p3 = b[j - 3] if 3 <= j <= n + 2 else 0
    cont = 0x80 <= x <= 0xBF
    if cont != (p1 >= 0xC0 or p2 >= 0xE0 or p3 >= 0xF0):
        return True
    return ((p1 in INVALID_BYTES and cont) or (p1 == 0xE0 and x < 0xA0) or (p1 == 0xED and x > 0x9F) or
            (p1 == 0xF0 and x < 0x90) or (p1 == 0xF4 and x > 0x8F))


def prefix_bad(b):
    """utf8_bad of an open TEXT message whose delivered bytes are b: an error at a position inside b."""
    return int(any(b[j] >= 0x80 or (j and b[j - 1] >= 0x80) for j in range(len(b))) and
               any(utf8_flagged(b, j) for j in range(len(b))))


def strict_ok(b):
    try:
        bytes(b).decode("utf-8", "strict")
        return 1
    except UnicodeDecodeError:
        return 0


def tail_word(b):
    """The last 3 bytes of b as the dword before the next byte (bits 31:24 the last one)."""
    return int.from_bytes(b"\0" + bytes(b[-3:]).rjust(3, b"\0"), "little")


ZERO_CARRY = dict.fromkeys(_lib.MSG_CARRY.names, 0)


class RefConn:
    """The connection's state by the contract: the fws_msg_carry fields, and --
    the oracle's own, never the device's -- the open message's bytes so far."""

    def __init__(self):
        self.carry = dict(ZERO_CARRY)
        self.body = b""

    def call(self, wire, cap=BIG, msg_cap=BIG, dst_cap=BIG, ctl_cap=BIG):
        wire = bytes(wire)
        all_frames, parse_status = ref_parse(wire)
        frames = all_frames[:cap]
        c = self.carry
        is_open, opcode, total_frames = c["open_opcode"] != 0, c["open_opcode"], c["open_frames"]
        body = bytearray(self.body)
        continued, first, start, nfrag = is_open, NONE, 0, 0
        dst, ctl, entries, units = bytearray(), bytearray(), [], []
        n_data, err_frame, err_status, resume = 0, NONE, 0, 0
        for i, f in enumerate(frames):
            end = f["hdr_off"] + f["hdr_len"] + f["plen"]
            if f["op"] >= 8:
                if not f["fin"] or f["plen"] > 125:
                    err_frame, err_status, resume = i, _lib.FWS_ERR_CONTROL_FRAME, f["hdr_off"]
                    break
                if f["trunc"]:
                    resume = f["hdr_off"]
                    break
                p = unmask(wire, f)
                entries.append(dict(off=len(ctl), len=len(p), first_frame=i, last_frame=i, n_data_frames=1,
                                    opcode=f["op"], utf8_ok=0, flags=0, pad=0))
                units.append((f["op"], p, 0, 1))
                ctl += p
                resume = end
                continue
            if f["trunc"]:                            # whole frames only: not gathered, counted or checked
                resume = f["hdr_off"]
                break
            if (f["op"] == 0) != is_open:
                err_frame, err_status, resume = i, _lib.FWS_ERR_SEQUENCE, f["hdr_off"]
                break
            if f["op"]:
                is_open, opcode, continued, first, start, nfrag = True, f["op"], False, i, len(dst), 0
                body, total_frames = bytearray(), 0
            elif first == NONE:
                first = i
            p = unmask(wire, f)
            dst += p
            body += p
            n_data, nfrag, total_frames, resume = n_data + 1, nfrag + 1, total_frames + 1, end
            if f["fin"]:
                ok = strict_ok(body) if opcode == TEXT else 0
                entries.append(dict(off=start, len=len(dst) - start, first_frame=first, last_frame=i,
                                    n_data_frames=nfrag, opcode=opcode, utf8_ok=ok,
                                    flags=CONTINUED if continued else 0, pad=0))
                units.append((opcode, bytes(body), ok, total_frames))
                is_open, continued, first, body, total_frames = False, False, NONE, bytearray(), 0
        deny = len(entries) > msg_cap or len(dst) > dst_cap or len(ctl) > ctl_cap
        status = err_status or parse_status or (_lib.FWS_ERR_CAPACITY if deny or len(all_frames) > cap else 0)
        res = dict(status=status, n_msgs=len(entries), err_frame=err_frame,
                   open_first_frame=first if is_open else NONE, open_opcode=opcode if is_open else 0,
                   n_data_frames=n_data, data_bytes=len(dst), ctl_bytes=len(ctl),
                   open_off=start if is_open else 0, open_len=len(dst) - start if is_open else 0,
                   resume_off=0 if deny else resume)
        text_open = is_open and opcode == TEXT
        new = dict(open_opcode=opcode if is_open else 0, open_frames=total_frames if is_open else 0,
                   open_bytes=len(body) if is_open else 0, utf8_tail=tail_word(body) if text_open else 0,
                   utf8_bad=prefix_bad(body) if text_open else 0, prev_open_opcode=c["open_opcode"],
                   prev_open_frames=c["open_frames"], prev_open_bytes=c["open_bytes"],
                   wire_bytes=c["wire_bytes"] + resume, n_msgs=c["n_msgs"] + len(entries), reserved=0)
        if deny:                                      # nothing delivered: the same bytes come again
            for e in entries:
                e["utf8_ok"] = 0
            dst, ctl, units, new = b"", b"", [], dict(c)
        else:
            self.carry, self.body = new, bytes(body) if is_open else b""
        return dict(dst=bytes(dst), ctl=bytes(ctl), entries=entries, units=units, res=res, carry=new,
                    n_frames=len(all_frames), err_hdr=c["wire_bytes"] + resume if err_status else None)


# ------------------------------------------------------------------ runner
def align(n, a=256):
    return (n + a - 1) // a * a


class Call:
    """One call's buffers in one device arena (every buffer followed by guard
    bytes), uploaded and fetched in one copy each; the carry is the caller's."""

    def __init__(self, cuda, wire, cap=None, msg_cap=None, dst_cap=None, ctl_cap=None):
        self.wire = wire = bytes(wire)
        n = len(wire)
        self.cap = n // 6 + 16 if cap is None else cap
        self.msg_cap = self.cap if msg_cap is None else msg_cap
        self.dst_cap = n + 16 if dst_cap is None else dst_cap
        self.ctl_cap = n + 16 if ctl_cap is None else ctl_cap
        sizes = dict(wire=max(n, 16), wire2=max(n, 16), dst=self.dst_cap, ctl=self.ctl_cap,
                     frames=self.cap * _lib.FRAME_INFO.itemsize, frames2=self.cap * _lib.FRAME_INFO.itemsize,
                     msgs=self.msg_cap * _lib.MSG_INFO.itemsize, res=_lib.DECODE_RESULT.itemsize,
                     res2=_lib.DECODE_RESULT.itemsize, mres=_lib.MSG_RESULT.itemsize)
        self.at, off = {}, 0
        for k, sz in sizes.items():
            self.at[k] = (off, sz)
            off = align(off + sz + GUARD)
        host = np.full(off, FILL, dtype=np.uint8)
        for k in ("wire", "wire2"):
            host[self.at[k][0]:self.at[k][0] + n] = np.frombuffer(wire, dtype=np.uint8)
        self.host_in = torch.from_numpy(host)
        self.arena = self.host_in.to(cuda)

    def t(self, k):
        o, sz = self.at[k]
        return self.arena[o:o + sz + GUARD]

    def launch(self, ctx, carry, with_stream=True):
        n = len(self.wire)
        rc, *_ = gpu.decode_messages_carry(ctx, self.t("wire"), self.cap, self.msg_cap, self.t("dst"), self.t("ctl"),
                                           carry, frames=self.t("frames"), msgs=self.t("msgs"), result=self.t("res"),
                                           msg_result=self.t("mres"), n=n, dst_cap=self.dst_cap,
                                           ctl_cap=self.ctl_cap)
        assert rc == 0, rc
        if with_stream:
            rc2, *_ = gpu.decode_stream(ctx, self.t("wire2"), cap=self.cap, frames=self.t("frames2"),
                                        result=self.t("res2"), n=n)
            assert rc2 == 0, rc2

    def check(self, ref, with_stream=True):
        """The fetched arena against the walk's output for this call."""
        got = self.arena.cpu().numpy()
        fill = bytes([FILL])

        def buf(k):
            o, sz = self.at[k]
            return got[o:o + sz + GUARD].tobytes()

        n = len(self.wire)
        assert buf("wire") == self.wire + fill * (max(n, 16) - n + GUARD), "the wire was modified"
        r = np.frombuffer(buf("mres")[:_lib.MSG_RESULT.itemsize], dtype=_lib.MSG_RESULT)[0]
        for k in _lib.MSG_RESULT.names:
            assert int(r[k]) == ref["res"][k], (k, int(r[k]), ref["res"][k])
        assert buf("mres")[_lib.MSG_RESULT.itemsize:] == fill * GUARD
        assert buf("dst") == ref["dst"] + fill * (self.dst_cap + GUARD - len(ref["dst"])), "dst"
        assert buf("ctl") == ref["ctl"] + fill * (self.ctl_cap + GUARD - len(ref["ctl"])), "ctl"
        ne, isz = min(len(ref["entries"]), self.msg_cap), _lib.MSG_INFO.itemsize
        em = np.frombuffer(buf("msgs")[:ne * isz], dtype=_lib.MSG_INFO)
        for i in range(ne):
            for k in _lib.MSG_INFO.names:
                assert int(em[i][k]) == ref["entries"][i][k], (i, k, int(em[i][k]), ref["entries"][i][k])
        assert buf("msgs")[ne * isz:] == fill * (self.msg_cap * isz + GUARD - ne * isz), "entries past the count"
        dsz = _lib.DECODE_RESULT.itemsize
        d = np.frombuffer(buf("res")[:dsz], dtype=_lib.DECODE_RESULT)[0]
        assert int(d["n_frames"]) == ref["n_frames"]
        assert buf("res")[dsz:] == fill * GUARD
        fsz = _lib.FRAME_INFO.itemsize
        assert buf("frames")[self.cap * fsz:] == fill * GUARD, "frames past cap"
        if with_stream:                               # what fws_gpu_decode_stream reports for the same bytes
            assert buf("res")[:dsz] == buf("res2")[:dsz]
            nf = min(ref["n_frames"], self.cap) * fsz
            assert buf("frames")[:nf] == buf("frames2")[:nf]
        return r


def new_carry(cuda, fields=None):
    host = np.full(_lib.MSG_CARRY.itemsize + GUARD, FILL, dtype=np.uint8)
    c = np.zeros(1, dtype=_lib.MSG_CARRY)
    for k, v in (fields or {}).items():
        c[0][k] = v
    host[:_lib.MSG_CARRY.itemsize] = c.view(np.uint8)
    return torch.from_numpy(host).to(cuda)


def check_carry(carry, want):
    raw = carry.cpu().numpy().tobytes()
    got = np.frombuffer(raw[:_lib.MSG_CARRY.itemsize], dtype=_lib.MSG_CARRY)[0]
    for k in _lib.MSG_CARRY.names:
        assert int(got[k]) == want[k], (k, int(got[k]), want[k])
    assert raw[_lib.MSG_CARRY.itemsize:] == bytes([FILL]) * GUARD, "bytes after the carry"
    return raw[:_lib.MSG_CARRY.itemsize]


class Conn:
    """A connection on the device and its reference, fed chunk by chunk."""

    def __init__(self, ctx, cuda):
        self.ctx, self.cuda, self.ref, self.carry = ctx, cuda, RefConn(), new_carry(cuda)
        self.units, self.calls, self.continued, self.last = [], 0, 0, None

    def call(self, wire, **caps):
        c = Call(self.cuda, wire, **caps)
        out = self.ref.call(wire, c.cap, c.msg_cap, c.dst_cap, c.ctl_cap)
        c.launch(self.ctx, self.carry)
        c.check(out)
        out["carry_bytes"] = check_carry(self.carry, out["carry"])
        self.units += out["units"]
        self.calls += 1
        self.continued += sum(1 for e in out["entries"] if e["flags"] & CONTINUED)
        self.last = out
        return out

    def feed(self, stream, cuts):
        """The stream cut at `cuts`: every call gets the bytes from the last resume_off up to the next cut."""
        pos = 0
        for b in sorted(set(cuts)) + [len(stream)]:
            out = self.call(stream[pos:b])
            pos += out["res"]["resume_off"]
            if out["res"]["status"] not in (0, _lib.FWS_ERR_CAPACITY):
                break
        return pos


def whole(stream):
    """The one-call decode of the whole stream by the walk: its units, status and failing header."""
    out = RefConn().call(stream)
    return out["units"], out["res"]["status"], out["err_hdr"]


def check_cut(ctx, cuda, stream, cuts):
    units, status, err_hdr = whole(stream)
    conn = Conn(ctx, cuda)
    conn.feed(stream, cuts)
    assert conn.units == units
    assert conn.last["res"]["status"] == status and conn.last["err_hdr"] == err_hdr
    return conn


def payload(rng, n):
    return bytes(rng.getrandbits(8) for _ in range(n))


def key(rng):
    return rng.getrandbits(32)


def message(rng, parts, opcode=BIN, fin=1):
    out = b""
    for j, p in enumerate(parts):
        out += frame(opcode if j == 0 else CONT, p, fin=1 if (j == len(parts) - 1 and fin) else 0, key=key(rng))
    return out


def frames_as_calls(rng, frames):
    """Each (opcode, payload, fin) a frame, each frame a call's bytes."""
    return [frame(op, p, fin=fin, key=key(rng)) for op, p, fin in frames]


def fragments(parts, opcode=TEXT):
    return [(opcode if j == 0 else CONT, p, int(j == len(parts) - 1)) for j, p in enumerate(parts)]


# ------------------------------------------------------------------ 1. zero carry = the old call
def good_messages(rng, n):
    out = b""
    for k in range(n):
        op = rng.choice((TEXT, BIN))
        parts = [payload(rng, rng.randint(0, 40)) if op == BIN else b"caf\xc3\xa9 " * rng.randint(0, 6)
                 for _ in range(1 + (k % 3 == 1) * 2)]
        out += message(rng, parts, op)
        if k % 4 == 3:
            out += frame(rng.choice((PING, PONG)), payload(rng, rng.randint(0, 30)), key=key(rng))
    return out


@pytest.mark.parametrize("seed", range(5))
def test_zero_carry_equals_the_old_call(ctx, cuda, seed):
    rng = random.Random(seed)
    wire = good_messages(rng, (1, 7, 40, 120, 300)[seed]) + frame(CLOSE, struct.pack(">H", 1000), key=key(rng))
    c = Call(cuda, wire)
    carry = new_carry(cuda)
    c.launch(ctx, carry)
    old = Call(cuda, wire)
    rc, *_ = gpu.decode_messages(ctx, old.t("wire"), old.cap, old.msg_cap, old.t("dst"), old.t("ctl"),
                                 frames=old.t("frames"), msgs=old.t("msgs"), result=old.t("res"),
                                 msg_result=old.t("mres"), n=len(wire), dst_cap=old.dst_cap, ctl_cap=old.ctl_cap)
    assert rc == 0
    ref = RefConn().call(wire)
    c.check(ref)
    check_carry(carry, ref["carry"])
    a, b = c.arena.cpu().numpy(), old.arena.cpu().numpy()
    for k in ("dst", "ctl", "msgs", "mres", "frames", "res"):
        o, sz = c.at[k]
        assert a[o:o + sz + GUARD].tobytes() == b[o:o + sz + GUARD].tobytes(), k


# ------------------------------------------------------------------ 2. cut at every byte
def twelve_frames():
    """TEXT in 3 fragments with a PING between them (the 2-, 4- and 10-byte
    length forms, a character split over the first seam), BIN in 2 with an
    empty fragment and a PONG inside, single-frame messages, a CLOSE."""
    rng = random.Random(2)
    f = [frame(TEXT, b"he\xe2\x82", fin=0, key=key(rng)),
         frame(PING, b"p1", key=key(rng)),
         frame(CONT, b"\xac and more", fin=0, key=key(rng), len_form=126),
         frame(CONT, b"the end \xf0\x9f\x98\x80", fin=1, key=key(rng), len_form=127),
         frame(BIN, b"\x00\xff\x80", fin=0, key=key(rng)),
         frame(CONT, b"", fin=0, key=key(rng)),
         frame(PONG, b"", key=key(rng)),
         frame(CONT, payload(rng, 10), fin=1, key=key(rng)),
         frame(TEXT, b"ok", key=key(rng)),
         frame(TEXT, b"bad \xc3(", key=key(rng)),
         frame(BIN, payload(rng, 17), key=key(rng), len_form=126),
         frame(CLOSE, struct.pack(">H", 1000) + b"bye", key=key(rng))]
    return b"".join(f)


def test_cut_in_two_at_every_byte(ctx, cuda):
    stream = twelve_frames()
    units, status, _ = whole(stream)
    assert [u[0] for u in units] == [PING, TEXT, PONG, BIN, TEXT, TEXT, BIN, CLOSE] and status == 0
    assert [u[2] for u in units] == [0, 1, 0, 0, 1, 0, 0, 0] and units[1][3] == 3 and units[3][3] == 3
    continued = 0
    for cut in range(len(stream) + 1):
        continued += check_cut(ctx, cuda, stream, [cut]).continued
    assert continued > 40


def test_cut_in_three_over_a_stride(ctx, cuda):
    stream = twelve_frames()
    for a in range(1, len(stream), 13):
        for b in range(a + 1, len(stream), 17):
            check_cut(ctx, cuda, stream, [a, b])


# ------------------------------------------------------------------ 3. UTF-8 across calls
VALID = ["é".encode(), "€".encode(), "\U0001F600".encode()]
ILL_FORMED = [b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"\xe0\x80\x80", b"\xc0\x80", b"\xff\xfe", b"\xf5\x80\x80\x80",
              b"\xe2\x28\xa1", b"\x80"]


def feed_frames(ctx, cuda, rng, frames):
    """Each frame its own call; returns the connection and the carry after each call."""
    conn, carries = Conn(ctx, cuda), []
    for w in frames_as_calls(rng, frames):
        carries.append(conn.call(w)["carry"])
    return conn, carries


@pytest.mark.parametrize("seq", VALID + ILL_FORMED, ids=lambda s: s.hex())
def test_sequence_split_at_every_position(ctx, cuda, seq):
    rng = random.Random(len(seq))
    want = strict_ok(b"ab" + seq + b"cd")
    assert want == (seq in VALID)
    for cut in range(1, len(seq)):                    # the call boundary at every position inside it
        conn, _ = feed_frames(ctx, cuda, rng, fragments([b"ab" + seq[:cut], seq[cut:] + b"cd"]))
        assert conn.units == [(TEXT, b"ab" + seq + b"cd", want, 2)]
    # a byte per call, with empty fragments between them: a 4-byte sequence spans six calls
    parts = [b"ab"]
    for i in range(len(seq)):
        parts += [seq[i:i + 1], b""] if i % 2 == 0 else [seq[i:i + 1]]
    conn, _ = feed_frames(ctx, cuda, rng, fragments(parts + [b"cd"]))
    assert conn.units == [(TEXT, b"ab" + seq + b"cd", want, len(parts) + 1)]
    # in three calls, the sequence's ends in the outer ones
    if len(seq) >= 3:
        conn, _ = feed_frames(ctx, cuda, rng, fragments([b"ab" + seq[:1], seq[1:-1], seq[-1:] + b"cd"]))
        assert conn.units == [(TEXT, b"ab" + seq + b"cd", want, 3)]
    # the sequence at the very end of the message, cut before its last byte
    conn, _ = feed_frames(ctx, cuda, rng, fragments([seq[:-1], seq[-1:]]))
    assert conn.units == [(TEXT, seq, strict_ok(seq), 2)]
    conn, _ = feed_frames(ctx, cuda, rng, fragments([b"ab" + seq[:-1], b""]))
    assert conn.units == [(TEXT, b"ab" + seq[:-1], strict_ok(b"ab" + seq[:-1]), 2)]


def test_utf8_bad_is_set_by_the_first_call_that_holds_a_complete_error(ctx, cuda):
    rng = random.Random(31)
    # ED A0: the second byte is out of ED's range -- complete with the second call
    conn, c = feed_frames(ctx, cuda, rng, fragments([b"a\xed", b"\xa0", b"\x80z", b"!"]))
    assert [x["utf8_bad"] for x in c] == [0, 1, 1, 0] and conn.units[0][2] == 0
    assert [x["utf8_tail"] for x in c[:3]] == [tail_word(b"a\xed"), tail_word(b"a\xed\xa0"), tail_word(b"\xa0\x80z")]
    # a lead byte whose continuation never comes: an error only once the next byte is there
    conn, c = feed_frames(ctx, cuda, rng, fragments([b"abc\xe2", b"", b"x", b""]))
    assert [x["utf8_bad"] for x in c] == [0, 0, 1, 0] and conn.units[0][2] == 0
    # an invalid byte as the last byte of a part: flagged at the byte after it, so by the next call
    conn, c = feed_frames(ctx, cuda, rng, fragments([b"ab\xc0", b"cd", b"ef"]))
    assert [x["utf8_bad"] for x in c] == [0, 1, 0] and conn.units[0][2] == 0
    conn, c = feed_frames(ctx, cuda, rng, fragments([b"ab\xff", b""]))        # ... or by the final verdict
    assert [x["utf8_bad"] for x in c] == [0, 0] and conn.units == [(TEXT, b"ab\xff", 0, 2)]
    # sticky: good bytes after the error do not clear it
    conn, c = feed_frames(ctx, cuda, rng, fragments([b"\x80", b"fine", b"fine", b"."]))
    assert [x["utf8_bad"] for x in c] == [1, 1, 1, 0] and conn.units[0][2] == 0
    # BIN carries no UTF-8 state
    conn, c = feed_frames(ctx, cuda, rng, fragments([b"\xff\xe2", b"\x82"], BIN))
    assert [(x["utf8_bad"], x["utf8_tail"]) for x in c] == [(0, 0), (0, 0)]


def test_the_tail_does_not_leak_into_the_next_message(ctx, cuda):
    rng = random.Random(32)
    conn = Conn(ctx, cuda)
    conn.call(frame(TEXT, b"ab", fin=0, key=key(rng)))
    out = conn.call(frame(CONT, b"\xe2\x82", fin=1, key=key(rng)) + frame(TEXT, b"\xac", key=key(rng)) +
                    frame(TEXT, b"\xe2", fin=0, key=key(rng)))
    assert [e["utf8_ok"] for e in out["entries"]] == [0, 0]
    assert out["carry"]["utf8_tail"] == tail_word(b"\xe2") and out["carry"]["utf8_bad"] == 0
    # the open message ends cut; the next one, in the same later call, starts with continuation bytes
    out = conn.call(frame(CONT, b"\x82", fin=1, key=key(rng)) + frame(TEXT, b"\xac", key=key(rng)))
    assert [e["utf8_ok"] for e in out["entries"]] == [0, 0]
    assert (out["carry"]["utf8_tail"], out["carry"]["utf8_bad"], out["carry"]["open_opcode"]) == (0, 0, 0)
    # together they would have been a valid character: "\xe2\x82" + "\xac"
    assert strict_ok(b"\xe2\x82\xac") == 1


# ------------------------------------------------------------------ 4. sequencing through the carry
def test_sequencing_at_the_first_frame_of_a_call(ctx, cuda):
    rng = random.Random(41)

    def opened():
        conn = Conn(ctx, cuda)
        conn.call(frame(TEXT, b"open", fin=0, key=key(rng)) + frame(PING, b"x", key=key(rng)))
        assert conn.ref.carry["open_opcode"] == TEXT
        return conn

    conn = opened()
    out = conn.call(frame(TEXT, b"new", key=key(rng)) + frame(BIN, b"later", key=key(rng)))
    assert (out["res"]["status"], out["res"]["err_frame"]) == (_lib.FWS_ERR_SEQUENCE, 0)
    assert out["entries"] == [] and out["res"]["resume_off"] == 0

    conn = Conn(ctx, cuda)
    out = conn.call(frame(CONT, b"stray", key=key(rng)))
    assert (out["res"]["status"], out["res"]["err_frame"]) == (_lib.FWS_ERR_SEQUENCE, 0)

    conn = opened()
    out = conn.call(frame(CONT, b" and closed", fin=1, key=key(rng)))
    assert out["res"]["status"] == 0 and conn.units[-1] == (TEXT, b"open and closed", 1, 2)
    assert out["entries"][0]["flags"] == CONTINUED and out["entries"][0]["off"] == 0

    conn = opened()
    before = dict(conn.ref.carry)
    out = conn.call(frame(PING, b"x", fin=0, key=key(rng)) + frame(CONT, b"", fin=1, key=key(rng)))
    assert (out["res"]["status"], out["res"]["err_frame"]) == (_lib.FWS_ERR_CONTROL_FRAME, 0)
    # the state just before frame 0: nothing moved (prev_open_* now mirror what this call found)
    for k in ("open_opcode", "open_frames", "open_bytes", "utf8_tail", "utf8_bad", "wire_bytes", "n_msgs"):
        assert out["carry"][k] == before[k], k
    assert out["res"]["open_opcode"] == TEXT and out["res"]["open_first_frame"] == NONE

    # an error later in the call: the carry is the state before it
    conn = opened()
    out = conn.call(frame(CONT, b"!", fin=0, key=key(rng)) + frame(BIN, b"new", key=key(rng)))
    assert (out["res"]["status"], out["res"]["err_frame"]) == (_lib.FWS_ERR_SEQUENCE, 1)
    assert (out["carry"]["open_opcode"], out["carry"]["open_bytes"], out["carry"]["open_frames"]) == (TEXT, 5, 2)


# ------------------------------------------------------------------ 5. the init state reaches every workgroup
def carried_open_conn(ctx, cuda, rng, first=b"\xe2"):
    conn = Conn(ctx, cuda)
    conn.call(frame(TEXT, first, fin=0, key=key(rng)))
    return conn


def test_17000_continuation_frames_behind_a_carried_message(ctx, cuda):
    """More than 64 planner workgroups of 256 frames: the look-back's second
    round meets the position before workgroup 0, which is the carry's state."""
    rng = random.Random(51)
    conn = carried_open_conn(ctx, cuda, rng)
    body = b"\x82\xac" + "€".encode() * 5665 + b"ab\xe2"
    assert len(body) == 17000
    wire = b"".join(frame(CONT, body[i:i + 1], fin=0, key=key(rng)) for i in range(17000))
    out = conn.call(wire + frame(CONT, b"\x82\xac!", fin=1, key=key(rng)))
    e = out["entries"][0]
    assert (e["flags"], e["off"], e["len"], e["first_frame"], e["last_frame"], e["n_data_frames"]) == \
        (CONTINUED, 0, 17003, 0, 17000, 17001)
    assert out["carry"]["prev_open_bytes"] + e["len"] == 17004 and out["carry"]["prev_open_frames"] == 1
    assert conn.units == [(TEXT, b"\xe2" + body + b"\x82\xac!", 1, 17002)]


@pytest.mark.parametrize("fin_at", [255, 256, 257, 600])
def test_fin_frame_in_a_later_workgroup(ctx, cuda, fin_at):
    rng = random.Random(fin_at)
    conn = carried_open_conn(ctx, cuda, rng, b"abc")
    wire = frame(PING, b"first", key=key(rng))
    wire += b"".join(frame(CONT, payload(rng, rng.randint(0, 9)), fin=0, key=key(rng)) for _ in range(fin_at - 1))
    wire += frame(CONT, b"fin", fin=1, key=key(rng))
    wire += b"".join(message(rng, [payload(rng, 5)] * 2, BIN) for _ in range(20))
    wire += frame(TEXT, b"left open", fin=0, key=key(rng))
    out = conn.call(wire)
    e = out["entries"][1]
    assert (e["flags"], e["off"], e["first_frame"], e["last_frame"], e["n_data_frames"]) == \
        (CONTINUED, 0, 1, fin_at, fin_at)
    assert conn.units[1][3] == fin_at + 1
    assert out["res"]["open_first_frame"] == fin_at + 41 and out["carry"]["open_bytes"] == 9
    assert all(x["flags"] == 0 for x in out["entries"][2:])


# ------------------------------------------------------------------ 6. calls with no data frame
def test_calls_without_a_data_frame(ctx, cuda):
    rng = random.Random(61)
    conn = carried_open_conn(ctx, cuda, rng, b"ab\xf0\x9f")
    before = dict(conn.ref.carry)
    assert before["utf8_tail"] == tail_word(b"ab\xf0\x9f")
    ping = frame(PING, b"are you there", key=key(rng))
    for wire in (ping, b"", ping[:10], ping[:5], ping[:1]):
        out = conn.call(wire)
        whole_frame = wire == ping
        assert out["res"]["open_opcode"] == TEXT and out["res"]["open_len"] == 0
        assert out["res"]["open_first_frame"] == NONE and out["res"]["resume_off"] == (len(ping) if whole_frame else 0)
        for k in ("open_opcode", "open_frames", "open_bytes", "utf8_tail", "utf8_bad"):
            assert out["carry"][k] == before[k], k
    assert conn.ref.carry["n_msgs"] == 1 and conn.ref.carry["wire_bytes"] == before["wire_bytes"] + len(ping)
    out = conn.call(frame(CONT, b"\x98\x80", fin=1, key=key(rng)))
    assert conn.units[-1] == (TEXT, "ab\U0001F600".encode(), 1, 2)
    # the same with nothing open
    conn = Conn(ctx, cuda)
    for wire in (b"", ping):
        out = conn.call(wire)
        assert out["res"]["open_opcode"] == 0 and out["carry"]["open_opcode"] == 0


# ------------------------------------------------------------------ 7. capacities
def capacity_stream(rng):
    wire = frame(TEXT, b"sp\xc3", fin=0, key=key(rng)) + frame(PING, b"in between", key=key(rng))
    tail = frame(CONT, b"\xa4t", fin=1, key=key(rng)) + good_messages(rng, 12)
    tail += frame(PONG, b"last control", key=key(rng)) + message(rng, [b"tail", b" end"], TEXT)
    tail += frame(BIN, b"open at the end", fin=0, key=key(rng))
    return wire, tail


def test_frame_capacity_is_continued_from_resume_off(ctx, cuda):
    rng = random.Random(71)
    head, tail = capacity_stream(rng)
    stream = head + tail
    units, status, _ = whole(stream)
    conn, pos, statuses = Conn(ctx, cuda), 0, []
    while pos < len(stream):
        out = conn.call(stream[pos:], cap=3)
        statuses.append(out["res"]["status"])
        assert out["res"]["resume_off"] > 0
        pos += out["res"]["resume_off"]
    assert set(statuses[:-1]) == {_lib.FWS_ERR_CAPACITY} and statuses[-1] == 0 and len(statuses) >= 5
    assert conn.units == units and status == 0 and conn.continued >= 1
    assert conn.ref.carry["open_opcode"] == BIN and conn.ref.carry["wire_bytes"] == len(stream)


@pytest.mark.parametrize("short", ["dst_cap", "ctl_cap", "msg_cap"])
def test_byte_and_entry_capacities_leave_the_carry_alone(ctx, cuda, short):
    rng = random.Random(72)
    head, tail = capacity_stream(rng)
    units, _, _ = whole(head + tail)
    conn = Conn(ctx, cuda)
    before = conn.call(head)
    full = RefConn()
    full.carry, full.body = dict(conn.ref.carry), conn.ref.body
    full = full.call(tail)
    kw = {"dst_cap": dict(dst_cap=full["res"]["data_bytes"] - 1), "ctl_cap": dict(ctl_cap=full["res"]["ctl_bytes"] - 1),
          "msg_cap": dict(msg_cap=full["res"]["n_msgs"] - 1)}[short]
    out = conn.call(tail, **kw)
    assert out["res"]["status"] == _lib.FWS_ERR_CAPACITY and out["res"]["resume_off"] == 0
    assert out["carry_bytes"] == before["carry_bytes"], "the carry moved"
    assert (out["dst"], out["ctl"]) == (b"", b"")                 # (Call.check: the buffers hold only fill)
    for k in ("n_msgs", "data_bytes", "ctl_bytes"):               # what to size the retry with
        assert out["res"][k] == full["res"][k]
    exact = dict(dst_cap=full["res"]["data_bytes"], ctl_cap=full["res"]["ctl_bytes"], msg_cap=full["res"]["n_msgs"])
    out = conn.call(tail, **exact)
    assert out["res"]["status"] == 0 and out["res"]["resume_off"] == len(tail)
    assert conn.units == units and out["entries"][0]["flags"] == CONTINUED


# ------------------------------------------------------------------ 8. random streams
def log_uniform(rng, hi):
    return int(math.exp(rng.uniform(0.0, math.log(hi + 1)))) - 1


def random_text(rng, n):
    """n bytes of well-formed UTF-8: characters of 1 to 4 bytes, ASCII where no longer one fits."""
    out = bytearray()
    while len(out) < n:
        ch = chr(rng.choice((rng.randint(0x20, 0x7E), rng.randint(0xA0, 0x7FF), rng.randint(0x800, 0xD7FF),
                             rng.randint(0x10000, 0x10FFFF)))).encode()
        out += ch if len(out) + len(ch) <= n else b"."
    return bytes(out)


def random_stream(seed):
    """test_random_streams' generator at a few KiB. Returns the wire, the frames'
    (start, end) and the fragmented messages as (first frame, last frame)."""
    rng = random.Random(seed)
    target = rng.randint(20, 60)
    wire, spans, fragmented = b"", [], []

    def put(b):
        nonlocal wire
        spans.append((len(wire), len(wire) + len(b)))
        wire += b

    while len(spans) < target:
        if rng.random() < 0.08:
            put(frame(rng.choice((PING, PONG)), payload(rng, rng.randint(0, 125)), key=key(rng)))
            continue
        n = log_uniform(rng, 700)
        op = rng.choice((TEXT, BIN))
        body = random_text(rng, n) if op == TEXT else payload(rng, n)
        if op == TEXT and n and rng.random() < 0.15:
            b = bytearray(body)
            b[rng.randrange(n)] = rng.choice((0xFF, 0xC0, 0x80, 0xED, 0xF5))
            body = bytes(b)
            if rng.random() < 0.5:
                body = body[:-1] + b"\xe2"
        parts = [body]
        if rng.random() < 0.40 or not fragmented:     # (the first message is always fragmented)
            k = rng.randint(2, 6)
            cuts = sorted(rng.randint(0, n) for _ in range(k - 1))
            parts = [body[a:b] for a, b in zip([0] + cuts, cuts + [n])]
            first = len(spans)
        for j, p in enumerate(parts):
            put(frame(op if j == 0 else CONT, p, fin=int(j == len(parts) - 1), key=key(rng)))
            if j + 1 < len(parts) and rng.random() < 0.08:
                put(frame(PING, payload(rng, rng.randint(0, 20)), key=key(rng)))
        if len(parts) > 1:
            fragmented.append((first, len(spans) - 1))
    return wire, spans, fragmented


def random_cuts(seed):
    """2 to 6 cut points: one inside a fragmented message -- after its first
    fragment, before the end of its FIN frame, so a part is delivered and the
    rest completes it in a later call --, one inside a frame, the rest anywhere."""
    wire, spans, fragmented = random_stream(seed)
    rng = random.Random(1000 + seed)
    first, last = rng.choice(fragmented)
    cuts = {rng.randint(spans[first][1], spans[last][1] - 1)}
    while True:
        a, b = rng.choice(spans)
        inside = rng.randint(a + 1, b - 1)            # (a frame is at least 6 bytes)
        if inside not in cuts:
            cuts.add(inside)
            break
    want = rng.randint(2, 6)
    while len(cuts) < want:
        cuts.add(rng.randint(1, len(wire) - 1))
    return wire, sorted(cuts)


def reference_walk(seed):
    """The reference alone over the seed's cuts: (calls made, CONTINUED entries delivered, units)."""
    wire, cuts = random_cuts(seed)
    ref, pos, calls, continued, units = RefConn(), 0, 0, 0, []
    for b in cuts + [len(wire)]:
        out = ref.call(wire[pos:b])
        pos += out["res"]["resume_off"]
        calls, units = calls + 1, units + out["units"]
        continued += sum(1 for e in out["entries"] if e["flags"] & CONTINUED)
    return calls, continued, units


@pytest.mark.parametrize("seed", range(40))
def test_random_streams(ctx, cuda, seed):
    wire, cuts = random_cuts(seed)
    assert 2 <= len(cuts) <= 6 and 400 < len(wire) < 8192
    conn = check_cut(ctx, cuda, wire, cuts)
    assert conn.calls >= 2 and conn.continued >= 1    # a condition on the inputs (checked for all seeds on the CPU)
    assert conn.last["res"]["status"] == 0 and conn.ref.carry["wire_bytes"] == len(wire)


# ------------------------------------------------------------------ 9. two calls, no host step between
def test_two_calls_queued_on_one_stream(ctx, cuda):
    rng = random.Random(91)
    a = good_messages(rng, 5) + frame(TEXT, b"gr\xc3", fin=0, key=key(rng)) + frame(PING, b"mid", key=key(rng))
    b = frame(CONT, b"\xbc\xc3", fin=0, key=key(rng)) + frame(CONT, b"\x9fe", fin=1, key=key(rng))
    b += good_messages(rng, 300) + frame(BIN, b"open", fin=0, key=key(rng))
    ref = RefConn()
    outs = [ref.call(a), ref.call(b)]                 # frame-aligned chunks: the host knows the offsets
    assert outs[0]["res"]["resume_off"] == len(a) and outs[1]["entries"][0]["flags"] == CONTINUED
    calls, carry = [Call(cuda, a), Call(cuda, b)], new_carry(cuda)
    torch.cuda.synchronize()
    for c in calls:
        c.launch(ctx, carry, with_stream=False)
    torch.cuda.synchronize()
    for c, out in zip(calls, outs):
        c.check(out, with_stream=False)
    check_carry(carry, outs[1]["carry"])
    assert outs[1]["units"][0] == (TEXT, "grüße".encode(), 1, 3)


# ------------------------------------------------------------------ 10. graph capture
def test_graph_capture_and_replay(cuda, resolve_mode):
    """One captured call over a fixed-size chunk buffer, replayed three times
    with the buffer refilled: the carry flows through the replays in device
    memory (no memset node, no host step), and the last one delivers the TEXT
    message that spans all three with its totals and verdict."""
    rng = random.Random(101)
    body = random_text(rng, 100) + "€".encode() + random_text(rng, 96) + "\U0001F600".encode() + random_text(rng, 100)
    parts = [body[:101], body[101:202], body[202:]]   # the characters split 1 + 2 and 3 + 1
    assert [strict_ok(p) for p in parts] == [0, 0, 0] and strict_ok(body)
    chunks = []
    for j, p in enumerate(parts):
        chunks.append(frame(TEXT if j == 0 else CONT, p, fin=int(j == 2), key=key(rng)) +
                      frame(PING, payload(rng, 9), key=key(rng)))
    assert len(set(map(len, chunks))) == 1
    n, cap = len(chunks[0]), 8
    ref = RefConn()
    outs = [ref.call(w, cap, cap, n, n) for w in chunks]
    assert outs[2]["units"][0][2:] == (1, 3) and outs[2]["entries"][0]["flags"] == CONTINUED
    c = gpu.Ctx(0)
    c.reserve(cap, n)
    try:
        call = Call(cuda, chunks[0], cap=cap, msg_cap=cap, dst_cap=n, ctl_cap=n)
        carry = new_carry(cuda)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            call.launch(c, carry, with_stream=False)
        carry.copy_(new_carry(cuda))
        for w, out in zip(chunks, outs):
            call.wire = w
            host = call.host_in.clone()
            host[call.at["wire"][0]:call.at["wire"][0] + n] = torch.from_numpy(np.frombuffer(w, dtype=np.uint8).copy())
            call.arena.copy_(host)
            g.replay()
            torch.cuda.synchronize()
            call.check(out, with_stream=False)
            check_carry(carry, out["carry"])
        e = outs[2]["entries"][0]
        assert (outs[2]["carry"]["prev_open_bytes"] + e["len"], outs[2]["carry"]["prev_open_frames"] +
                e["n_data_frames"]) == (303, 3)
    finally:
        torch.cuda.synchronize()
        c.close()


# ------------------------------------------------------------------ 11. MessageStream
@pytest.mark.parametrize("seed", [3, 17])
def test_message_stream_returns_the_reference_units(ctx, cuda, seed):
    wire, _, _ = random_stream(seed)
    units, status, _ = whole(wire)
    assert status == 0
    rng = random.Random(seed)
    ms = gpu.MessageStream(ctx, max_read=700, max_frame=2048)
    got, pos, feeds = [], 0, 0
    while pos < len(wire):
        k = rng.randint(1, 700)
        got += ms.feed(wire[pos:pos + k])
        pos, feeds = pos + k, feeds + 1
    assert got == [(op, body, bool(ok)) for op, body, ok, _ in units]
    assert ms.status == 0 and feeds >= 2
    c = gpu.read_msg_carry(ms.carry)
    assert int(c["wire_bytes"]) == len(wire) and int(c["n_msgs"]) == len(units) and int(c["open_opcode"]) == 0
