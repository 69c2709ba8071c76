"""GPU parity of fws_gpu_decode_messages (parse -> message planner -> gather ->
control payloads -> UTF-8 of the reassembled TEXT messages), bit-exact against
a pure-Python reference written here: the wire is walked with struct, unmasked
with the key bytes, grouped by FIN and opcode (RFC 6455 §5.4, §5.5) and TEXT
messages are validated with bytes.decode("utf-8", "strict").

Every case compares dst, ctl, every fws_msg_info and fws_msg_result field and
the guard bytes after each buffer, checks the wire byte-for-byte unchanged, and
compares dev_frames / dev_result with fws_gpu_decode_stream on a copy."""
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


def ref_messages(wire, cap, msg_cap, dst_cap, ctl_cap):
    wire = bytes(wire)
    all_frames, parse_status = ref_parse(wire)
    frames = all_frames[:cap]
    dst, ctl, entries = bytearray(), bytearray(), []
    is_open, first, opcode, start, nfrag = False, NONE, 0, 0, 0
    n_data, err_frame, err_status = 0, NONE, 0
    resume = 0
    for i, f in enumerate(frames):
        end = min(f["hdr_off"] + f["hdr_len"] + f["plen"], len(wire))
        if f["op"] >= 8:
            if not f["fin"] or f["plen"] > 125:
                err_frame, err_status = i, _lib.FWS_ERR_CONTROL_FRAME
                resume = f["hdr_off"]
                break
            if f["trunc"]:
                resume = f["hdr_off"]
                break
            entries.append(dict(off=len(ctl), len=f["plen"], first_frame=i, last_frame=i, n_data_frames=1,
                                opcode=f["op"], utf8_ok=0, flags=0, pad=0))
            ctl += unmask(wire, f)
            resume = end
            continue
        if (f["op"] == 0) != is_open:
            err_frame, err_status = i, _lib.FWS_ERR_SEQUENCE
            resume = f["hdr_off"]
            break
        if f["op"]:
            is_open, first, opcode, start, nfrag = True, i, f["op"], len(dst), 0
        dst += unmask(wire, f)
        n_data += 1
        nfrag += 1
        resume = end
        if f["fin"] and not f["trunc"]:
            body = bytes(dst[start:])
            ok = 0
            if opcode == TEXT:
                try:
                    body.decode("utf-8", "strict")
                    ok = 1
                except UnicodeDecodeError:
                    ok = 0
            entries.append(dict(off=start, len=len(body), first_frame=first, last_frame=i, n_data_frames=nfrag,
                                opcode=opcode, utf8_ok=ok, flags=0, pad=0))
            is_open = False
    if is_open:
        resume = frames[first]["hdr_off"]
    over = (len(all_frames) > cap or len(entries) > msg_cap or len(dst) > dst_cap or len(ctl) > ctl_cap)
    status = err_status or parse_status or (_lib.FWS_ERR_CAPACITY if over else 0)
    if len(dst) > dst_cap:                           # nothing gathered: no verdicts
        for e in entries:
            e["utf8_ok"] = 0
    res = dict(status=status, n_msgs=len(entries), err_frame=err_frame,
               open_first_frame=first if is_open else NONE, open_opcode=opcode if is_open else 0,
               n_data_frames=n_data, data_bytes=len(dst), ctl_bytes=len(ctl),
               open_off=start if is_open else 0, open_len=len(dst) - start if is_open else 0, resume_off=resume)
    return dict(dst=bytes(dst) if len(dst) <= dst_cap else b"", ctl=bytes(ctl) if len(ctl) <= ctl_cap else b"",
                entries=entries, res=res, n_frames=len(all_frames))


# ------------------------------------------------------------------ runner
def guarded(n, cuda):
    return torch.full((n + GUARD,), FILL, dtype=torch.uint8, device=cuda)


def run(ctx, cuda, wire, cap=None, msg_cap=None, dst_cap=None, ctl_cap=None):
    wire = bytes(wire)
    cap = len(wire) // 6 + 16 if cap is None else cap
    msg_cap = cap if msg_cap is None else msg_cap
    dst_cap = len(wire) + 16 if dst_cap is None else dst_cap
    ctl_cap = len(wire) + 16 if ctl_cap is None else ctl_cap
    host = np.frombuffer(wire, dtype=np.uint8)
    dev = torch.from_numpy(host.copy()).to(cuda) if len(wire) else torch.zeros(16, dtype=torch.uint8, device=cuda)
    dst, ctl = guarded(dst_cap, cuda), guarded(ctl_cap, cuda)
    frames = guarded(cap * _lib.FRAME_INFO.itemsize, cuda)
    msgs = guarded(msg_cap * _lib.MSG_INFO.itemsize, cuda)
    rc, fr, ms, res, mres = gpu.decode_messages(ctx, dev, cap, msg_cap, dst, ctl, frames=frames, msgs=msgs,
                                                n=len(wire), dst_cap=dst_cap, ctl_cap=ctl_cap)
    assert rc == 0, rc
    ref = compare(wire, dev, cap, msg_cap, dst_cap, ctl_cap, dst, ctl, fr, ms, res, mres)
    # dev_frames / dev_result: what fws_gpu_decode_stream reports for the same bytes
    dev2 = torch.from_numpy(host.copy()).to(cuda) if len(wire) else torch.zeros(16, dtype=torch.uint8, device=cuda)
    rc2, fr2, res2, _ = gpu.decode_stream(ctx, dev2, cap=cap, n=len(wire))
    assert rc2 == 0
    r, r2 = gpu.read_result(res), gpu.read_result(res2)
    for k in _lib.DECODE_RESULT.names:
        assert r[k] == r2[k], k
    n = min(int(r["n_frames"]), cap)
    assert gpu.read_frames(fr, n).tobytes() == gpu.read_frames(fr2, n).tobytes()
    return ref, gpu.read_msg_result(mres)


def compare(wire, dev, cap, msg_cap, dst_cap, ctl_cap, dst, ctl, fr, ms, res, mres):
    ref = ref_messages(wire, cap, msg_cap, dst_cap, ctl_cap)
    torch.cuda.synchronize()
    assert dev[:len(wire)].cpu().numpy().tobytes() == wire, "the wire was modified"
    got = gpu.read_msg_result(mres)
    for k in _lib.MSG_RESULT.names:
        assert int(got[k]) == ref["res"][k], (k, int(got[k]), ref["res"][k])
    assert int(gpu.read_result(res)["n_frames"]) == ref["n_frames"]
    fill = bytes([FILL])
    assert dst.cpu().numpy().tobytes() == ref["dst"] + fill * (dst_cap + GUARD - len(ref["dst"])), "dst"
    assert ctl.cpu().numpy().tobytes() == ref["ctl"] + fill * (ctl_cap + GUARD - len(ref["ctl"])), "ctl"
    n = min(len(ref["entries"]), msg_cap)
    em = gpu.read_messages(ms, n)
    for i in range(n):
        for k in _lib.MSG_INFO.names:
            assert int(em[i][k]) == ref["entries"][i][k], (i, k, int(em[i][k]), ref["entries"][i][k])
    isz = _lib.MSG_INFO.itemsize
    assert ms[n * isz:].cpu().numpy().tobytes() == fill * (ms.numel() - n * isz), "entries past the count"
    fsz = _lib.FRAME_INFO.itemsize
    assert fr[cap * fsz:].cpu().numpy().tobytes() == fill * GUARD, "frames past cap"
    return ref


def payload(rng, n):
    return bytes(rng.getrandbits(8) for _ in range(n))


def key(rng):
    return rng.getrandbits(32)


def message(rng, parts, opcode=BIN, fin=1):
    """One message as frames: parts = the fragments' payloads."""
    out = b""
    for j, p in enumerate(parts):
        out += frame(opcode if j == 0 else CONT, p, fin=1 if (j == len(parts) - 1 and fin) else 0, key=key(rng))
    return out


# ------------------------------------------------------------------ planner boundaries
FRAME_COUNTS = [1, 63, 64, 65, 255, 256, 257, 1025]


@pytest.mark.parametrize("nf", FRAME_COUNTS)
def test_one_frame_per_message(ctx, cuda, nf):
    rng = random.Random(nf)
    wire = b"".join(message(rng, [payload(rng, rng.randint(0, 40))], rng.choice((TEXT, BIN))) for _ in range(nf))
    ref, got = run(ctx, cuda, wire)
    assert ref["res"]["n_msgs"] == nf and ref["res"]["status"] == 0


@pytest.mark.parametrize("nf", FRAME_COUNTS)
def test_three_fragments_per_message(ctx, cuda, nf):
    """Frames 3k, 3k + 1, 3k + 2 form a message: at 255 / 256 / 257 frames a
    message's first frame and its FIN frame fall in different planner
    workgroups; a frame count that is no multiple of 3 leaves a message open."""
    rng = random.Random(1000 + nf)
    wire = b""
    for f in range(nf):
        wire += frame(BIN if f % 3 == 0 else CONT, payload(rng, rng.randint(0, 40)), fin=int(f % 3 == 2),
                      key=key(rng))
    ref, got = run(ctx, cuda, wire)
    assert ref["res"]["n_msgs"] == nf // 3
    assert (ref["res"]["open_first_frame"] == NONE) == (nf % 3 == 0)


def test_message_spanning_three_workgroups(ctx, cuda):
    rng = random.Random(7)
    wire = b"".join(message(rng, [payload(rng, rng.randint(0, 40))], TEXT) for _ in range(100))
    wire += message(rng, [payload(rng, rng.randint(0, 40)) for _ in range(600)], BIN)   # frames 100 .. 699
    wire += b"".join(message(rng, [payload(rng, rng.randint(0, 40))], BIN) for _ in range(10))
    ref, got = run(ctx, cuda, wire)
    e = ref["entries"][100]
    assert (e["first_frame"], e["last_frame"], e["n_data_frames"]) == (100, 699, 600)


# ------------------------------------------------------------------ gather seams
SEAM_LENS = [0, 1, 15, 16, 17, 4095, 4096, 4097]


@pytest.mark.parametrize("lead", [7, 9, 15])
def test_fragment_length_pairs(ctx, cuda, lead):
    """Every ordered pair of the seam lengths adjacent in one message, behind a
    first frame that shifts the source alignment."""
    rng = random.Random(lead)
    parts = [payload(rng, lead)]
    for a in SEAM_LENS:
        for b in SEAM_LENS:
            parts += [payload(rng, a), payload(rng, b)]
    ref, got = run(ctx, cuda, message(rng, parts, BIN))
    assert ref["res"]["n_msgs"] == 1 and ref["entries"][0]["n_data_frames"] == len(parts)


def test_long_fragment_and_unit_ends(ctx, cuda):
    """A 70,000-B fragment (64-bit length form), a message that ends exactly on a
    4 KiB dst unit and one that ends one byte past the next."""
    rng = random.Random(70000)
    wire = message(rng, [payload(rng, 5000), payload(rng, 3192)], BIN)            # dst [0, 8192)
    wire += message(rng, [payload(rng, 4097)], BIN)                              # ends at 12289
    wire += message(rng, [payload(rng, 9), payload(rng, 70000), payload(rng, 17)], TEXT)
    ref, got = run(ctx, cuda, wire)
    assert [e["off"] + e["len"] for e in ref["entries"][:2]] == [8192, 12289]
    assert ref["res"]["n_msgs"] == 3


# ------------------------------------------------------------------ UTF-8 across fragment seams
def text_msg(rng, parts, opcode=TEXT):
    return message(rng, parts, opcode)


def test_valid_sequences_split_at_every_byte(ctx, cuda):
    rng = random.Random(11)
    wire, n = b"", 0
    for seq in ("é".encode(), "€".encode(), "\U0001F600".encode()):
        for cut in range(1, len(seq)):
            wire += text_msg(rng, [seq[:cut], seq[cut:]])
            n += 1
        wire += text_msg(rng, [seq[i:i + 1] for i in range(len(seq))])
        wire += text_msg(rng, [b"ab" + seq[:1], seq[1:] + b"cd"])
        n += 2
    ref, got = run(ctx, cuda, wire)
    assert [e["utf8_ok"] for e in ref["entries"]] == [1] * n


def test_invalid_sequences_split_at_the_seam(ctx, cuda):
    rng = random.Random(12)
    wire = text_msg(rng, [b"\xed", b"\xa0\x80"]) + text_msg(rng, [b"\xf4", b"\x90\x80\x80"])
    wire += text_msg(rng, [b"\xe0", b"\x80\x80"])
    wire += text_msg(rng, [b"abc", b"\xe2"])                         # ends in a bare lead byte
    wire += text_msg(rng, [b"\xff\xfe", b"\xc0"], BIN)               # BIN: no verdict, no error
    wire += text_msg(rng, [b"fine"])
    ref, got = run(ctx, cuda, wire)
    assert [e["utf8_ok"] for e in ref["entries"]] == [0, 0, 0, 0, 0, 1]
    assert ref["res"]["status"] == 0


def test_context_does_not_leak_across_messages(ctx, cuda):
    """Messages are adjacent in dst: the 3-byte left context of a message's first
    bytes must be empty, whatever the previous message ended with."""
    rng = random.Random(13)
    wire = text_msg(rng, [b"ab\xf0\x9f\x98"]) + text_msg(rng, [b"hello"])       # invalid, then valid
    wire += text_msg(rng, [b"\xf0\x9f\x98"]) + text_msg(rng, [b"\x80"])         # together valid, each invalid
    wire += text_msg(rng, [b"\xe2\x82"], BIN) + text_msg(rng, [b"\xac"])        # BIN lead bytes, TEXT continuation
    ref, got = run(ctx, cuda, wire)
    assert [e["utf8_ok"] for e in ref["entries"]] == [0, 1, 0, 0, 0, 0]


# ------------------------------------------------------------------ control frames
def test_control_frames_between_fragments_and_messages(ctx, cuda):
    rng = random.Random(21)
    p = [payload(rng, n) for n in (300, 5, 4096, 33)]
    close = struct.pack(">H", 1000) + b"bye"
    wire = frame(TEXT, b"one", key=key(rng))
    wire += frame(PING, b"", key=key(rng))                                        # an empty PING
    wire += frame(BIN, p[0], fin=0, key=key(rng))
    wire += frame(PING, payload(rng, 125), key=key(rng))                          # a 125-B PING
    wire += frame(CONT, p[1], fin=0, key=key(rng))
    wire += frame(PONG, b"pong", key=key(rng))
    wire += frame(CONT, p[2], fin=0, key=key(rng))
    wire += frame(CONT, p[3], fin=1, key=key(rng))
    wire += frame(PONG, b"between", key=key(rng))
    wire += frame(TEXT, b"two", key=key(rng))
    wire += frame(CLOSE, close, key=key(rng))
    ref, got = run(ctx, cuda, wire)
    assert [e["opcode"] for e in ref["entries"]] == [TEXT, PING, PING, PONG, BIN, PONG, TEXT, CLOSE]
    big = ref["entries"][4]
    assert (big["first_frame"], big["last_frame"], big["n_data_frames"]) == (2, 7, 4)
    assert ref["dst"][big["off"]:big["off"] + big["len"]] == b"".join(p)          # contiguous
    assert ref["ctl"].endswith(close)


def test_close_between_fragments(ctx, cuda):
    rng = random.Random(22)
    wire = frame(TEXT, b"he", fin=0, key=key(rng)) + frame(CLOSE, struct.pack(">H", 1001) + b"going away",
                                                           key=key(rng))
    wire += frame(CONT, b"llo", fin=1, key=key(rng))
    ref, got = run(ctx, cuda, wire)
    assert [e["opcode"] for e in ref["entries"]] == [CLOSE, TEXT]


# ------------------------------------------------------------------ sequencing errors
def good_messages(rng, n, k0=0):
    out = b""
    for k in range(k0, k0 + n):
        parts = [payload(rng, rng.randint(0, 40)) for _ in range(1 + (k % 3 == 1) * 2)]
        out += message(rng, parts, BIN)
        if k % 7 == 3:
            out += frame(PING, b"p", key=key(rng))
    return out


def frames_of(wire):
    return len(ref_parse(wire)[0])


BAD = {
    "continuation_first": lambda rng: (frame(CONT, b"stray", fin=1, key=key(rng)), 0, _lib.FWS_ERR_SEQUENCE),
    "text_while_open": lambda rng: (frame(BIN, b"open", fin=0, key=key(rng)) + frame(TEXT, b"new", key=key(rng)),
                                    1, _lib.FWS_ERR_SEQUENCE),
    "control_without_fin": lambda rng: (frame(PING, b"x", fin=0, key=key(rng)), 0, _lib.FWS_ERR_CONTROL_FRAME),
    "control_126_bytes": lambda rng: (frame(PING, payload(rng, 126), key=key(rng)), 0,
                                      _lib.FWS_ERR_CONTROL_FRAME),
}


def prefix_for(rng, where):
    if where == "first":
        return b""
    if where == "after_three":
        return good_messages(rng, 3)
    pre, k = b"", 0                                   # the error at frame 300: a later planner workgroup
    while frames_of(pre) < 290:
        pre += good_messages(rng, 1, k)
        k += 1
    while frames_of(pre) < 300:
        pre += frame(BIN, b"pad", key=key(rng))
    return pre


@pytest.mark.parametrize("where", ["first", "after_three", "frame_300"])
@pytest.mark.parametrize("kind", list(BAD))
def test_sequencing_errors(ctx, cuda, kind, where):
    rng = random.Random(sorted(BAD).index(kind) * 10 + len(where))
    pre = prefix_for(rng, where)
    bad, rel, status = BAD[kind](rng)
    wire = pre + bad + good_messages(rng, 4)          # what follows the error is not delivered
    ref, got = run(ctx, cuda, wire)
    e = frames_of(pre) + rel
    if where == "frame_300":
        assert e == 300 + rel
    assert ref["res"]["err_frame"] == e and ref["res"]["status"] == status
    assert all(m["last_frame"] < e for m in ref["entries"])


def test_parse_error_after_good_messages(ctx, cuda):
    rng = random.Random(31)
    wire = good_messages(rng, 5) + frame(3, b"bad opcode", key=key(rng)) + good_messages(rng, 2)
    ref, got = run(ctx, cuda, wire)
    assert ref["res"]["status"] == _lib.FWS_ERR_OPCODE and ref["res"]["err_frame"] == NONE
    assert ref["res"]["n_msgs"] > 5


def test_sequencing_error_comes_before_a_later_parse_error(ctx, cuda):
    rng = random.Random(32)
    wire = good_messages(rng, 2) + frame(CONT, b"stray", key=key(rng)) + frame(3, b"bad", key=key(rng))
    ref, got = run(ctx, cuda, wire)
    assert ref["res"]["status"] == _lib.FWS_ERR_SEQUENCE


# ------------------------------------------------------------------ stream ends
def test_open_message_at_the_end(ctx, cuda):
    rng = random.Random(41)
    wire = good_messages(rng, 3) + frame(TEXT, b"\xe2\x82", fin=0, key=key(rng)) + frame(PING, b"hi", key=key(rng))
    wire += frame(CONT, b"\xac more", fin=0, key=key(rng))
    ref, got = run(ctx, cuda, wire)
    assert ref["res"]["open_opcode"] == TEXT and ref["res"]["open_len"] == 8
    assert ref["entries"][-1]["opcode"] == PING


def test_empty_stream(ctx, cuda):
    ref, got = run(ctx, cuda, b"")
    assert ref["res"] == dict(status=0, n_msgs=0, err_frame=NONE, open_first_frame=NONE, open_opcode=0,
                              n_data_frames=0, data_bytes=0, ctl_bytes=0, open_off=0, open_len=0, resume_off=0)


@pytest.mark.parametrize("cut", ["payload", "fin_payload", "header", "control_payload", "first_header"])
def test_truncated_end_and_resume(ctx, cuda, cut):
    """The stream ends inside a payload / a header; resubmitting wire[resume_off:]
    plus the missing tail yields the completed message."""
    rng = random.Random(len(cut))
    head = good_messages(rng, 4)
    parts = [payload(rng, 700), payload(rng, 300), payload(rng, 50)]
    f = [frame(TEXT, parts[0], fin=0, key=key(rng)), frame(CONT, parts[1], fin=0, key=key(rng)),
         frame(PING, b"ping", key=key(rng)), frame(CONT, parts[2], fin=1, key=key(rng))]
    tail = good_messages(rng, 2)
    full = head + b"".join(f) + tail
    at = {"payload": len(head) + len(f[0]) + 100,                 # inside the second fragment
          "fin_payload": len(head) + len(b"".join(f)) - 10,       # inside the FIN fragment
          "header": len(head) + len(f[0]) + len(f[1]) + len(f[2]) + 3,
          "control_payload": len(head) + len(f[0]) + len(f[1]) + 8,
          "first_header": len(head) + 1}[cut]
    ref, got = run(ctx, cuda, full[:at])
    resume = ref["res"]["resume_off"]
    assert resume == len(head)
    if cut != "first_header":
        assert ref["res"]["open_first_frame"] != NONE
    ref2, got2 = run(ctx, cuda, full[resume:])
    assert ref2["entries"][0]["opcode"] == PING
    first = ref2["entries"][1]
    assert first["opcode"] == TEXT and ref2["dst"][first["off"]:first["off"] + first["len"]] == b"".join(parts)
    assert ref2["res"]["status"] == 0 and ref2["res"]["resume_off"] == len(full) - resume


def test_truncated_control_frame_is_not_delivered(ctx, cuda):
    rng = random.Random(43)
    head = good_messages(rng, 2)
    wire = head + frame(PING, b"0123456789", key=key(rng))[:-3]
    ref, got = run(ctx, cuda, wire)
    alone = ref_messages(head, 1 << 20, 1 << 20, 1 << 20, 1 << 20)
    assert ref["res"]["resume_off"] == len(head)
    assert (ref["res"]["n_msgs"], ref["ctl"]) == (alone["res"]["n_msgs"], alone["ctl"])


# ------------------------------------------------------------------ capacities
def capacity_stream(rng):
    wire = good_messages(rng, 12)
    wire += frame(PONG, b"last control", key=key(rng)) + message(rng, [b"tail", b" end"], TEXT)
    return wire


@pytest.mark.parametrize("short", ["cap", "msg_cap", "dst_cap", "ctl_cap"])
def test_capacities(ctx, cuda, short):
    rng = random.Random(51)
    wire = capacity_stream(rng)
    full = ref_messages(wire, 1 << 20, 1 << 20, 1 << 20, 1 << 20)
    kw = {"cap": dict(cap=full["n_frames"] - 3),
          "msg_cap": dict(msg_cap=full["res"]["n_msgs"] - 2),
          "dst_cap": dict(dst_cap=full["res"]["data_bytes"] - 1),
          "ctl_cap": dict(ctl_cap=full["res"]["ctl_bytes"] - 1)}[short]
    ref, got = run(ctx, cuda, wire, **kw)
    assert ref["res"]["status"] == _lib.FWS_ERR_CAPACITY
    if short != "cap":
        for k in ("n_msgs", "data_bytes", "ctl_bytes", "n_data_frames"):
            assert ref["res"][k] == full["res"][k]
    if short == "dst_cap":
        assert ref["dst"] == b"" and ref["ctl"] == full["ctl"]
    if short == "ctl_cap":
        assert ref["ctl"] == b"" and ref["dst"] == full["dst"]


def test_exact_capacities_are_enough(ctx, cuda):
    rng = random.Random(52)
    wire = capacity_stream(rng)
    full = ref_messages(wire, 1 << 20, 1 << 20, 1 << 20, 1 << 20)
    ref, got = run(ctx, cuda, wire, cap=full["n_frames"], msg_cap=full["res"]["n_msgs"],
                   dst_cap=full["res"]["data_bytes"], ctl_cap=full["res"]["ctl_bytes"])
    assert ref["res"]["status"] == 0


# ------------------------------------------------------------------ random streams
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
    rng = random.Random(seed)
    target = rng.randint(50, 600)
    wire, nf = b"", 0
    while nf < target:
        if rng.random() < 0.05:
            wire += frame(rng.choice((PING, PONG, CLOSE)), payload(rng, rng.randint(0, 125)), key=key(rng))
            nf += 1
            continue
        n = log_uniform(rng, 20000)
        op = rng.choice((TEXT, BIN))
        body = random_text(rng, n) if op == TEXT else payload(rng, n)
        if op == TEXT and n and rng.random() < 0.10:
            b = bytearray(body)
            b[rng.randrange(n)] = rng.choice((0xFF, 0xC0, 0x80, 0xED, 0xF5))
            body = bytes(b)
            if rng.random() < 0.5:
                body = body[:-1] + b"\xe2"
        parts = [body]
        if rng.random() < 0.30:
            k = rng.randint(2, 6)
            cuts = sorted(rng.randint(0, n) for _ in range(k - 1))
            parts = [body[a:b] for a, b in zip([0] + cuts, cuts + [n])]
        for j, p in enumerate(parts):
            wire += frame(op if j == 0 else CONT, p, fin=int(j == len(parts) - 1), key=key(rng))
            nf += 1
            if j + 1 < len(parts) and rng.random() < 0.05:
                wire += frame(PING, payload(rng, rng.randint(0, 20)), key=key(rng))
                nf += 1
    return wire


@pytest.mark.parametrize("seed", range(40))
def test_random_streams(ctx, cuda, seed):
    wire = random_stream(seed)
    ref, got = run(ctx, cuda, wire)
    assert ref["res"]["status"] == 0 and ref["res"]["n_msgs"] > 0


# ------------------------------------------------------------------ graph capture
def same_shape_streams():
    """Two streams of equal length and frame sizes that differ in every payload
    byte, key, FIN grouping and UTF-8 validity."""
    sizes = [0, 3, 17, 4096, 130, 70, 5000, 1, 64, 900] * 30
    out = []
    for seed in (1, 2):
        rng = random.Random(100 + seed)
        wire, is_open = b"", False
        for j, n in enumerate(sizes):
            if j % 11 == 5:
                wire += frame(PING, payload(rng, min(n, 125)), key=key(rng))
                continue
            fin = int(rng.random() < 0.5 or j == len(sizes) - 1)
            body = random_text(rng, n) if rng.random() < 0.7 else payload(rng, n)
            wire += frame(CONT if is_open else TEXT, body, fin=fin, key=key(rng))
            is_open = not fin
        out.append(wire)
    assert len(out[0]) == len(out[1])
    return out


def test_graph_capture_and_replay(cuda, resolve_mode):
    """After fws_gpu_ctx_reserve one call is captured and replayed on fresh
    inputs: the capture succeeds (no allocation, no host synchronisation -- both
    fail a stream capture) and each replay equals the reference, as the eager
    call does. Everything the call issues is on the one stream it is given."""
    a, b = same_shape_streams()
    n = len(a)
    cap = msg_cap = 400
    c = gpu.Ctx(0)
    c.reserve(cap, n)
    try:
        dev = torch.zeros(n, dtype=torch.uint8, device=cuda)
        dst, ctl = guarded(n, cuda), guarded(n, cuda)
        frames = guarded(cap * _lib.FRAME_INFO.itemsize, cuda)
        msgs = guarded(msg_cap * _lib.MSG_INFO.itemsize, cuda)
        res = torch.zeros(_lib.DECODE_RESULT.itemsize, dtype=torch.uint8, device=cuda)
        mres = torch.zeros(_lib.MSG_RESULT.itemsize, dtype=torch.uint8, device=cuda)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            rc, *_ = gpu.decode_messages(c, dev, cap, msg_cap, dst, ctl, frames=frames, msgs=msgs, result=res,
                                         msg_result=mres, n=n, dst_cap=n, ctl_cap=n)
        assert rc == 0
        for wire in (a, b, a):
            dev.copy_(torch.from_numpy(np.frombuffer(wire, dtype=np.uint8).copy()))
            for t in (dst, ctl, frames, msgs):
                t.fill_(FILL)
            g.replay()
            compare(wire, dev, cap, msg_cap, n, n, dst, ctl, frames, msgs, res, mres)
        # the eager call on the same context and buffers gives the same
        for t in (dst, ctl, frames, msgs):
            t.fill_(FILL)
        dev.copy_(torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()))
        rc, *_ = gpu.decode_messages(c, dev, cap, msg_cap, dst, ctl, frames=frames, msgs=msgs, result=res,
                                     msg_result=mres, n=n, dst_cap=n, ctl_cap=n)
        assert rc == 0
        compare(b, dev, cap, msg_cap, n, n, dst, ctl, frames, msgs, res, mres)
    finally:
        torch.cuda.synchronize()
        c.close()
