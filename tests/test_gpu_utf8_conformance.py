"""Device-side UTF-8 conformance: the corpus of utf8_corpus.py (Unicode Table
3-7, judged by Python's strict decoder) through every kernel that compiles
utf8_err in (fws_device.h):

  fws_gpu_validate_utf8            k_utf8<false>
  fws_gpu_unmask_sorted_utf8       k_unmask_sorted_utf8, 3 forms, + k_utf8_seam_sorted
  fws_gpu_decode_stream            k_unmask_stream<utf8>, prefetch on / off, + k_utf8_seam
  fws_gpu_decode_messages          k_utf8_msgs<false>
  fws_gpu_decode_messages_carry    k_utf8_msgs<true>
  fws_gpu_decode_messages_multi    the in-register check of k_msg_multi, both forms

A. values: corpus E (411,393 strings) through each validator;
B. values across calls: corpus E16 at every interior cut, two launches;
C. plumbing: corpus S placed on every seam of each validator's walk.

Every comparison is element-wise against the cached reference; where a call
also unmasks, the bytes are compared with the plain text."""
import functools

import numpy as np
import pytest
import torch

import utf8_corpus as uc
from flashws_amd import _lib, gpu
from test_gpu_msg_carry import RefConn
from wsframes import frame

pytestmark = pytest.mark.gpu

# the kernels' geometry (fws_device.h, msg_multi_kernels.hip)
CHUNK = 16                       # bytes a lane holds: one 16-B load
LANES = 64                       # lanes of a wave
STEP = CHUNK * LANES             # 1 KiB: a wave step
UNIT = 4096                      # a wave unit of the byte-space unmask kernels: 4 steps
MULTI = {"small": dict(max_len=16 << 10, threads=256, read=12000),          # k_msg_multi<16 KiB, 256>
         "full": dict(max_len=128 << 10, threads=1024, read=100000)}        # k_msg_multi<128 KiB, 1024>
MAX_FRAMES = _lib.FWS_MSG_MULTI_MAX_FRAMES
PARTS = 4                        # the (s, j) cases of a long-bodied test are dealt over this many test cases
TEXT, BIN, CONT = 1, 2, 0
CONTINUED = _lib.FWS_MSG_CONTINUED

V = frozenset(uc.seq_v())
S = uc.seq_s()
# one well-formed and one ill-formed sequence per length
REPRESENTATIVES = (b"\xc2\x80", b"\xe0\xa0\x80", b"\xf0\x90\x80\x80", b"\x80", b"\xc0\x80", b"\xe0\x9f\xbf",
                   b"\xf0\x8f\xbf\xbf")


# ------------------------------------------------------------------ fixtures
@pytest.fixture(params=[0, 1, 2], ids=["plain", "pipe", "early"])
def sorted_form(request):
    """the three forms of k_unmask_sorted_utf8"""
    L = _lib.lib()
    old = L.fws_internal_set_sorted_utf8_pipe(request.param)
    yield request.param
    L.fws_internal_set_sorted_utf8_pipe(old)


@pytest.fixture(params=[1, 0], ids=["pf", "no_pf"])
def stream_pf(request):
    """k_unmask_stream<utf8> with and without the cross-unit prefetch"""
    L = _lib.lib()
    old = L.fws_internal_set_stream_utf8_pf(request.param)
    yield request.param
    L.fws_internal_set_stream_utf8_pf(old)


# ------------------------------------------------------------------ comparing
def report(got, exp, describe):
    """got == exp element-wise, or the first few offenders by describe(i)."""
    got = np.asarray(got)
    assert len(got) == len(exp), (len(got), len(exp))
    assert np.isin(got, (0, 1)).all(), "a flag was not written"
    bad = np.nonzero(got.astype(bool) != exp)[0]
    if bad.size:
        lines = [f"  {describe(int(i))}: got {int(got[i])}, want {int(exp[i])}" for i in bad[:8]]
        pytest.fail(f"{bad.size} of {len(exp)} verdicts wrong, the first:\n" + "\n".join(lines), pytrace=False)


def same_bytes(got, want, what):
    if not np.array_equal(got, want):
        at = int(np.nonzero(got != want)[0][0])
        pytest.fail(f"{what}: byte {at} is {int(got[at]):02x}, want {int(want[at]):02x}", pytrace=False)


def e_describe(e, offs, layout):
    return lambda i: f"string {i} = [{e.string(i).hex()}] at byte {int(offs[i])} (phase {int(offs[i]) & 3}, {layout})"


class Case:
    """One region / frame / message of a plumbing test: its plain bytes, Python's
    verdict, the member of S it carries, where, and where the layout must put
    it: (lo + q) % mod == r for align = (q, mod, r)."""

    def __init__(self, body, ok, seq, note, align=None, gap=8):
        self.body, self.ok, self.seq, self.note, self.align, self.gap = body, ok, seq, note, align, gap


def check_cases(cases, got, where=lambda i: ""):
    exp = np.array([c.ok for c in cases])
    in_v = np.array([c.seq in V for c in cases])
    # not vacuous: well-formed exactly where the sequence is a member of V, and both kinds present
    assert int(exp.sum()) == int(in_v.sum()) > 0 and int((~exp).sum()) == int((~in_v).sum()) > 0
    assert np.array_equal(exp, in_v)
    report(got, exp, lambda i: f"case {i}: {cases[i].note} {where(i)}")


def seam_cases(total, q, seqs=S, align=None, what="the seam"):
    """For every sequence s and every j in 0..len(s): a body of `total` bytes in which byte j of
    s is the byte at offset q (j = 0: s starts at the seam; j = len(s): s ends on the byte before)."""
    out = []
    for s in seqs:
        for j in range(len(s) + 1):
            start = q - j
            assert start >= 0 and start + len(s) <= total
            body, ok = uc.s_case(start, s, total - start - len(s))
            out.append(Case(body, ok, s, f"[{s.hex()}] byte {j} first past {what} (body offset {q} of {total})", align))
    return out


def head_cases(total, seqs=S, align=None):
    return [Case(*uc.s_case(0, s, total - len(s)), s, f"[{s.hex()}] first bytes of {total}", align) for s in seqs]


def tail_cases(total, seqs=S, align=None):
    return [Case(*uc.s_case(total - len(s), s, 0), s, f"[{s.hex()}] last bytes of {total}", align) for s in seqs]


# ------------------------------------------------------------------ descriptor layouts (validate, sorted)
def place_regions(cases, seed):
    """The cases' bodies in one buffer in order, each at the first offset >= the
    previous end + its gap that satisfies its alignment. The bytes between are
    hostile: continuation bytes behind a region, lead bytes in front of the next."""
    rng = np.random.default_rng(seed)
    conts, leads = np.frombuffer(b"\x80\xbf", dtype=np.uint8), np.frombuffer(b"\xc2\xe2\xf0\xf4", dtype=np.uint8)
    parts, offs, pos = [], [], 0
    for k, c in enumerate(cases):
        lo = pos + (c.gap if k else 0)
        if c.align:
            q, mod, r = c.align
            lo += (r - (lo + q)) % mod
        g = lo - pos
        parts.append(conts[rng.integers(0, 2, g // 2)].tobytes() + leads[rng.integers(0, 4, g - g // 2)].tobytes())
        parts.append(c.body)
        offs.append(lo)
        pos = lo + len(c.body)
    parts.append(conts[rng.integers(0, 2, 32 + (-pos) % 16)].tobytes())
    buf = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
    assert len(buf) % 16 == 0
    return buf, np.array(offs, dtype=np.int64), np.array([len(c.body) for c in cases], dtype=np.int64)


def make_descs(offs, lens, keys=None, phases=None):
    d = np.zeros(len(offs), dtype=gpu.FRAME_DESC)
    d["payload_off"], d["payload_len"] = offs, lens
    if keys is not None:
        d["key"], d["phase"] = keys, phases
    return d


def random_keys(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(1, 2**32, n, dtype=np.uint64).astype(np.uint32), rng.integers(0, 4, n).astype(np.uint32))


def mask_regions(buf, offs, lens, keys, phases):
    """Every region XORed with its key at its phase, region by region (long regions)."""
    out = buf.copy()
    for o, n, k, ph in zip(offs.tolist(), lens.tolist(), keys.tolist(), phases.tolist()):
        kb = np.frombuffer(int(k).to_bytes(4, "little") * 2, dtype=np.uint8)[ph:ph + 4]
        out[o:o + n] ^= np.resize(kb, n)
    return out


def run_validate(ctx, cuda, buf, offs, lens):
    dev = torch.from_numpy(buf).to(cuda)
    ok = torch.full((len(offs),), 7, dtype=torch.uint8, device=cuda)
    gpu.validate_utf8(ctx, dev, gpu.descs_to_device(make_descs(offs, lens), cuda), len(offs), ok)
    torch.cuda.synchronize()
    same_bytes(dev.cpu().numpy(), buf, "fws_gpu_validate_utf8 wrote to the buffer")
    return ok.cpu().numpy()


def run_sorted(ctx, cuda, plain, masked, offs, lens, keys, phases):
    dev = torch.from_numpy(masked).to(cuda)
    ok = torch.full((len(offs),), 7, dtype=torch.uint8, device=cuda)
    gpu.unmask_sorted_utf8(ctx, dev, gpu.descs_to_device(make_descs(offs, lens, keys, phases), cuda), len(offs), ok)
    torch.cuda.synchronize()
    same_bytes(dev.cpu().numpy(), plain, "bytes after fws_gpu_unmask_sorted_utf8")
    return ok.cpu().numpy()


# ------------------------------------------------------------------ wire layouts (stream, messages, multi)
def short_frames(data, lens, opcodes, fins, seed):
    """One client frame per row (payloads of at most 4 bytes: 6-byte headers, random
    non-zero keys), vectorised. Returns (wire, the same with plain payloads, frame starts)."""
    n = len(lens)
    keys, _ = random_keys(n, seed)
    starts = np.concatenate([[0], np.cumsum(6 + lens)]).astype(np.int64)
    total = int(starts[-1])
    wire = np.zeros((total + 15) // 16 * 16, dtype=np.uint8)
    s = starts[:-1]
    wire[s] = (np.asarray(fins, dtype=np.uint8) << 7) | np.asarray(opcodes, dtype=np.uint8)
    wire[s + 1] = 0x80 | lens.astype(np.uint8)
    for k in range(4):
        wire[s + 2 + k] = ((keys >> np.uint32(8 * k)) & 0xFF).astype(np.uint8)
    plain = wire.copy()
    for k in range(4):
        m = lens > k
        plain[s[m] + 6 + k] = data[m, k]
        wire[s[m] + 6 + k] = data[m, k] ^ ((keys[m] >> np.uint32(8 * k)) & 0xFF).astype(np.uint8)
    return wire, plain, starts


def frame_pair(opcode, body, fin, key):
    """(the client frame, the same with its payload plain) for a payload of any length."""
    n = len(body)
    b0 = (fin << 7) | opcode
    if n < 126:
        hdr = bytes([b0, 0x80 | n])
    elif n < 65536:
        hdr = bytes([b0, 0x80 | 126]) + n.to_bytes(2, "big")
    else:
        hdr = bytes([b0, 0x80 | 127]) + n.to_bytes(8, "big")
    kb = int(key).to_bytes(4, "little")
    masked = (np.frombuffer(body, dtype=np.uint8) ^ np.resize(np.frombuffer(kb, dtype=np.uint8), n)).tobytes()
    return hdr + kb + masked, hdr + kb + body


def hdr_len(n):
    return 6 if n < 126 else (8 if n < 65536 else 14)


def place_frames(cases, seed):
    """The cases as FIN TEXT frames of one stream, each payload where its alignment
    asks (in stream bytes), BIN frames of hostile bytes making up the distance.
    Returns (wire, plain wire, the cases' frame indices, the frame count)."""
    rng = np.random.default_rng(seed)
    hostile = np.frombuffer(uc.HOSTILE, dtype=np.uint8)
    w, p, idx, pos, nf = [], [], [], 0, 0

    def put(opcode, body):
        nonlocal pos, nf
        a, b = frame_pair(opcode, body, 1, int(rng.integers(1, 2**32)))
        w.append(a)
        p.append(b)
        pos, nf = pos + len(a), nf + 1

    for c in cases:
        if c.align:
            q, mod, r = c.align
            d = (r - (pos + hdr_len(len(c.body)) + q)) % mod
            while d and (d < 6 or d in (132, 133)):      # no frame has that size
                d += mod
            if d:
                put(BIN, hostile[rng.integers(0, len(hostile), d - (6 if d < 132 else 8))].tobytes())
            assert (pos + hdr_len(len(c.body)) + q) % mod == r
        idx.append(nf)
        put(TEXT, c.body)
    pad = bytes((-pos) % 16)
    return (np.frombuffer(b"".join(w) + pad, dtype=np.uint8).copy(), np.frombuffer(b"".join(p) + pad, dtype=np.uint8).copy(),
            np.array(idx), nf, pos)


def run_stream(ctx, cuda, wire, plain, n, n_frames):
    dev = torch.from_numpy(wire).to(cuda)
    flags = torch.full((n_frames + 4,), 7, dtype=torch.uint8, device=cuda)
    rc, _, res, _ = gpu.decode_stream(ctx, dev, cap=n_frames + 4, utf8_ok=flags, n=n)
    assert rc == 0, rc
    r = gpu.read_result(res)
    assert (int(r["status"]), int(r["n_frames"]), int(r["consumed"])) == (0, n_frames, n)
    same_bytes(dev.cpu().numpy(), plain, "the stream after fws_gpu_decode_stream")
    return flags.cpu().numpy()[:n_frames]


def run_messages(ctx, cuda, wire, n, n_frames, n_msgs, carry=False):
    """fws_gpu_decode_messages, or (carry) fws_gpu_decode_messages_carry with a new connection's zero carry."""
    dev = torch.from_numpy(wire).to(cuda)
    dst = torch.zeros(len(wire) + 16, dtype=torch.uint8, device=cuda)
    ctl = torch.zeros(64, dtype=torch.uint8, device=cuda)
    if carry:
        rc, _, msgs, res, mres = gpu.decode_messages_carry(ctx, dev, n_frames + 4, n_msgs + 4, dst, ctl,
                                                           zero_carries(cuda, 1), n=n)
    else:
        rc, _, msgs, res, mres = gpu.decode_messages(ctx, dev, n_frames + 4, n_msgs + 4, dst, ctl, n=n)
    assert rc == 0, rc
    r, m = gpu.read_result(res), gpu.read_msg_result(mres)
    assert (int(r["status"]), int(r["n_frames"])) == (0, n_frames)
    assert (int(m["status"]), int(m["n_msgs"]), int(m["open_opcode"])) == (0, n_msgs, 0)
    same_bytes(dev.cpu().numpy(), wire, "fws_gpu_decode_messages wrote to the wire")
    return gpu.read_messages(msgs, n_msgs), dst.cpu().numpy(), int(m["data_bytes"])


def run_multi(ctx, cuda, wire, woff, lens, caps, dst_caps, max_len, carries):
    """One fws_gpu_decode_messages_multi launch: read r is wire[woff[r]:][:lens[r]] of connection
    r, its dst at the same offset, caps[r] frame and entry records. carries: the device carry
    array. Returns (fws_msg_result records, all entry records, entry bases, dst)."""
    n = len(lens)
    base = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
    desc = np.zeros(n, dtype=_lib.MSG_READ)
    desc["wire_off"] = desc["dst_off"] = woff
    desc["len"], desc["conn"], desc["dst_cap"], desc["ctl_cap"] = lens, np.arange(n), dst_caps, 16
    desc["frame_base"] = desc["msg_base"] = base[:-1]
    desc["frame_cap"] = desc["msg_cap"] = caps
    assert int(lens.max()) <= max_len and len(wire) % 16 == 0 and not (woff & 15).any()
    assert int((woff + np.maximum(dst_caps, (lens + 15) // 16 * 16)).max()) <= len(wire)
    u8 = dict(dtype=torch.uint8, device=cuda)
    dev = torch.from_numpy(wire).to(cuda)
    reads = torch.from_numpy(desc.view(np.uint8).copy()).to(cuda)
    dst, ctl = torch.zeros(len(wire), **u8), torch.zeros(64, **u8)
    frames = torch.zeros(int(base[-1]) * _lib.FRAME_INFO.itemsize, **u8)
    msgs = torch.zeros(int(base[-1]) * _lib.MSG_INFO.itemsize, **u8)
    res, mres = torch.zeros(n * _lib.DECODE_RESULT.itemsize, **u8), torch.zeros(n * _lib.MSG_RESULT.itemsize, **u8)
    rc = gpu.decode_messages_multi(ctx, dev, reads, n, max_len, frames, msgs, dst, ctl, res, mres, carries, n)
    assert rc == 0, rc
    torch.cuda.synchronize()
    m = np.frombuffer(mres.cpu().numpy().tobytes(), dtype=_lib.MSG_RESULT)
    bad = np.nonzero(m["status"] != 0)[0]
    assert bad.size == 0, f"read {int(bad[0])}: status {int(m['status'][bad[0]])} ({bad.size} reads not 0)"
    ent = np.frombuffer(msgs.cpu().numpy().tobytes(), dtype=_lib.MSG_INFO)
    return m, ent, base[:-1], dst.cpu().numpy()


def run_carry_each(ctx, cuda, wire, woff, lens, cap, dst_caps, carries):
    """The same reads one by one through fws_gpu_decode_messages_carry, `cap` frame and entry
    records each: what run_multi returns for them."""
    n = len(lens)
    u8 = dict(dtype=torch.uint8, device=cuda)
    csz, esz, rsz = _lib.MSG_CARRY.itemsize, _lib.MSG_INFO.itemsize, _lib.MSG_RESULT.itemsize
    dev = torch.from_numpy(wire).to(cuda)
    dst, ctl = torch.zeros(len(wire), **u8), torch.zeros(64, **u8)
    frames, res = torch.zeros(cap * _lib.FRAME_INFO.itemsize, **u8), torch.zeros(_lib.DECODE_RESULT.itemsize, **u8)
    msgs, mres = torch.zeros(n * cap * esz, **u8), torch.zeros(n * rsz, **u8)
    for r in range(n):
        o, ln, dc = int(woff[r]), int(lens[r]), int(dst_caps[r])
        rc, *_ = gpu.decode_messages_carry(ctx, dev[o:o + (ln + 15) // 16 * 16], cap, cap, dst[o:o + dc], ctl,
                                           carries[r * csz:(r + 1) * csz], frames=frames,
                                           msgs=msgs[r * cap * esz:(r + 1) * cap * esz], result=res,
                                           msg_result=mres[r * rsz:(r + 1) * rsz], n=ln, dst_cap=dc, ctl_cap=64)
        assert rc == 0, rc
    torch.cuda.synchronize()
    m = np.frombuffer(mres.cpu().numpy().tobytes(), dtype=_lib.MSG_RESULT)
    assert (m["status"] == 0).all()
    ent = np.frombuffer(msgs.cpu().numpy().tobytes(), dtype=_lib.MSG_INFO)
    return m, ent, cap * np.arange(n), dst.cpu().numpy()


def lay_reads(wires):
    """The reads in one host buffer, each at a 16-B aligned offset with at least 16 spare bytes: (buffer, offsets, lengths)."""
    lens = np.array([len(x) for x in wires], dtype=np.int64)
    slot = (lens + 15) // 16 * 16 + 16
    woff = np.concatenate([[0], np.cumsum(slot)[:-1]])
    host = np.zeros(int(slot.sum()), dtype=np.uint8)
    for r, x in enumerate(wires):
        host[woff[r]:woff[r] + lens[r]] = np.frombuffer(x, dtype=np.uint8)
    return host, woff, lens


def check_dst(dst, woff, plains, what):
    """Every read's data bytes at its dst_off are the plain payloads, and no other byte of dst was written."""
    want = np.zeros(len(dst), dtype=np.uint8)
    for o, p in zip(woff.tolist(), plains):
        want[o:o + len(p)] = np.frombuffer(p, dtype=np.uint8)
    same_bytes(dst, want, what)


def zero_carries(cuda, n):
    return torch.zeros(n * _lib.MSG_CARRY.itemsize, dtype=torch.uint8, device=cuda)


def read_carries(carries):
    return np.frombuffer(carries.cpu().numpy().tobytes(), dtype=_lib.MSG_CARRY)


# ================================================================== A. values: corpus E
@pytest.mark.parametrize("shift", range(4))
def test_values_validate_slots(ctx, cuda, shift):
    """k_utf8<false>: every string in a 4-byte slot at dword phase `shift` (all four over the
    parameter), a quarter of them across a 16-B lane seam; the slot's other bytes are hostile
    (sel_bytes must drop them)."""
    e = uc.corpus_e()
    buf, offs = uc.layout_slots(e, shift)
    report(run_validate(ctx, cuda, buf, offs, e.lens), e.ok, e_describe(e, offs, f"slots, shift {shift}"))


def test_values_validate_packed(ctx, cuda):
    """k_utf8<false>: the strings back to back, zero-length regions among them; every
    region's neighbours are other regions' bytes."""
    e = uc.corpus_e()
    buf, offs = uc.layout_packed(e)
    report(run_validate(ctx, cuda, buf, offs, e.lens), e.ok, e_describe(e, offs, "packed"))


@pytest.mark.parametrize("shift", range(4))
def test_values_sorted_slots(ctx, cuda, sorted_form, shift):
    """k_unmask_sorted_utf8 (utf8_slow_chunk: many regions per unit) + k_utf8_seam_sorted, random keys and phases."""
    e = uc.corpus_e()
    buf, offs = uc.layout_slots(e, shift)
    keys, phases = random_keys(len(e), 11 + shift)
    masked = uc.mask_strings(buf, e, offs, keys, phases)
    got = run_sorted(ctx, cuda, buf, masked, offs, e.lens, keys, phases)
    report(got, e.ok, e_describe(e, offs, f"slots, shift {shift}, form {sorted_form}"))


def test_values_sorted_packed(ctx, cuda, sorted_form):
    """Several regions, and the 3-byte tails of earlier ones, on every 4 KiB unit seam:
    k_utf8_seam_sorted's backwards loop over the regions that meet a seam, and utf8_slow_chunk."""
    e = uc.corpus_e()
    buf, offs = uc.layout_packed(e)
    keys, phases = random_keys(len(e), 17)
    masked = uc.mask_strings(buf, e, offs, keys, phases)
    got = run_sorted(ctx, cuda, buf, masked, offs, e.lens, keys, phases)
    report(got, e.ok, e_describe(e, offs, f"packed, form {sorted_form}"))


@functools.lru_cache(maxsize=None)
def e_wire():
    """Corpus E as one FIN TEXT frame per string."""
    e = uc.corpus_e()
    n = len(e)
    return short_frames(e.data, e.lens, np.full(n, TEXT), np.ones(n, dtype=np.uint8), seed=23)


@functools.lru_cache(maxsize=None)
def e_wire_fragmented():
    """Corpus E, every string of length >= 2 as TEXT fin=0 + CONT fin=1, split after byte 1 + (i mod (len - 1))."""
    e = uc.corpus_e()
    n = len(e)
    i = np.arange(n)
    split = e.lens >= 2
    k = np.where(split, 1 + i % np.maximum(e.lens - 1, 1), e.lens)
    first = i + np.concatenate([[0], np.cumsum(split)[:-1]])
    nf = n + int(split.sum())
    data, lens = np.zeros((nf, 4), dtype=np.uint8), np.zeros(nf, dtype=np.int64)
    ops, fins = np.full(nf, TEXT), np.ones(nf, dtype=np.uint8)
    col = np.arange(4)
    data[first] = np.where(col[None, :] < k[:, None], e.data, 0)
    lens[first] = k
    fins[first[split]] = 0
    second = first[split] + 1
    ops[second] = CONT
    lens[second] = (e.lens - k)[split]
    for kk in (1, 2, 3):
        m = split & (k == kk)
        data[first[m] + 1, :4 - kk] = e.data[m, kk:]
    return short_frames(data, lens, ops, fins, seed=29) + (nf,)


def test_values_decode_stream(ctx, cuda, stream_pf):
    """k_unmask_stream<utf8> + k_utf8_seam: one FIN TEXT frame per string, 6-byte headers, so
    the strings meet every chunk phase and the unit seams of the stream."""
    e = uc.corpus_e()
    wire, plain, starts = e_wire()
    got = run_stream(ctx, cuda, wire, plain, int(starts[-1]), len(e))
    report(got, e.ok, e_describe(e, starts[:-1] + 6, f"stream, prefetch {stream_pf}"))


@pytest.mark.parametrize("fragmented", [False, True], ids=["whole", "fragmented"])
def test_values_decode_messages(ctx, cuda, fragmented):
    """k_utf8_msgs<false> (utf8_region_bad<false>): one message per string, dst the packed
    layout; fragmented: the check runs on the gathered bytes of two frames."""
    e = uc.corpus_e()
    if fragmented:
        wire, _, starts, nf = e_wire_fragmented()
    else:
        (wire, _, starts), nf = e_wire(), len(e)
    ent, dst, nbytes = run_messages(ctx, cuda, wire, int(starts[-1]), nf, len(e))
    packed, offs = uc.layout_packed(e)
    assert nbytes == int(e.lens.sum())
    same_bytes(dst[:nbytes], packed[:nbytes], "dst")
    assert np.array_equal(ent["off"], offs) and np.array_equal(ent["len"], e.lens) and (ent["opcode"] == TEXT).all()
    if fragmented:
        assert np.array_equal(ent["n_data_frames"], 1 + (e.lens >= 2))
    report(ent["utf8_ok"], e.ok, e_describe(e, offs, "dst of decode_messages"))


@pytest.mark.parametrize("form", list(MULTI))
def test_values_decode_messages_multi(ctx, cuda, form):
    """k_msg_multi's in-register check: the frames of corpus E in reads of 256 frames, one
    connection with a zero carry per read, one launch."""
    e = uc.corpus_e()
    wire, _, starts = e_wire()
    first = np.arange(0, len(e), MAX_FRAMES)
    cnt = np.minimum(MAX_FRAMES, len(e) - first)
    lens = starts[first + cnt] - starts[first]
    slot = (lens + 15) // 16 * 16 + 16
    woff = np.concatenate([[0], np.cumsum(slot)[:-1]])
    host = np.zeros(int(slot.sum()), dtype=np.uint8)
    for r in range(len(first)):
        host[woff[r]:woff[r] + lens[r]] = wire[starts[first[r]]:starts[first[r]] + lens[r]]
    m, ent, base, dst = run_multi(ctx, cuda, host, woff, lens, np.full(len(first), MAX_FRAMES + 1), lens + 16,
                                  MULTI[form]["max_len"], zero_carries(cuda, len(first)))
    assert np.array_equal(m["n_msgs"], cnt) and (m["open_opcode"] == 0).all()
    packed, offs = uc.layout_packed(e)                # a read's dst: its strings back to back
    ends = np.concatenate([offs, [int(e.lens.sum())]])
    assert np.array_equal(m["data_bytes"], ends[first + cnt] - ends[first])
    check_dst(dst, woff, [packed[ends[a]:ends[a + c]].tobytes() for a, c in zip(first.tolist(), cnt.tolist())],
              f"dst of the reads, {form} form")
    got = np.concatenate([ent["utf8_ok"][base[r]:base[r] + cnt[r]] for r in range(len(first))])
    report(got, e.ok, e_describe(e, starts[:-1] + 6, f"stream byte; {form} form, reads of {MAX_FRAMES} frames"))


# ================================================================== B. values across calls: corpus E16
def tiny_reads(pay, plen, b0, seed):
    """One frame of at most 4 payload bytes per 16-byte slot: (wire, offsets, lengths)."""
    n = len(plen)
    keys, _ = random_keys(n, seed)
    w = np.zeros((n, 16), dtype=np.uint8)
    w[:, 0], w[:, 1] = b0, 0x80 | plen.astype(np.uint8)
    for k in range(4):
        kb = ((keys >> np.uint32(8 * k)) & 0xFF).astype(np.uint8)
        w[:, 2 + k] = kb
        w[:, 6 + k] = np.where(plen > k, pay[:, k] ^ kb, 0)
    return w.reshape(-1), 16 * np.arange(n, dtype=np.int64), 6 + plen


@functools.lru_cache(maxsize=None)
def e16_pairs():
    """(string, cut) for every interior cut of every string of E16; the two parts as rows."""
    c = uc.corpus_e16()
    sidx = np.repeat(np.arange(len(c)), c.lens - 1)
    cut = np.concatenate([np.arange(1, n) for n in c.lens.tolist()])
    assert len(sidx) == 256 * 1 + 4096 * 2 + 65536 * 3 == 205056
    col = np.arange(4)
    head = np.where(col[None, :] < cut[:, None], c.data[sidx], 0).astype(np.uint8)
    tail = np.zeros_like(head)
    for k in (1, 2, 3):
        m = cut == k
        tail[m, :4 - k] = c.data[sidx[m], k:]
    return c, sidx, cut, head, tail, c.lens[sidx] - cut


FIRST_PART_CARRY = {}            # first part -> RefConn's (utf8_tail, utf8_bad) after it: computed once per part


@pytest.mark.parametrize("part", range(PARTS))
def test_cross_call_values(ctx, cuda, part):
    """Corpus E16 at every interior cut through fws_gpu_decode_messages_multi (the 205,056
    (string, cut) connections dealt over PARTS test cases, two launches each): call 1 delivers
    TEXT fin=0 with the first part, call 2 CONT fin=1 with the rest. The carry after call 1
    (utf8_tail, utf8_bad: the prefix-mode check and the tail rebuild) is RefConn's; the verdict
    after call 2 (the seeded left context, the sticky error) is Python's on the whole string.
    A 1-in-64 sample of the same pairs goes through fws_gpu_decode_messages_carry
    (k_utf8_msgs<true>) and must give the same carries, entries and results."""
    c, sidx, cut, head, tail, tlen = e16_pairs()
    assert len(sidx) == 205056
    sidx, cut, head, tail, tlen = (x[part::PARTS] for x in (sidx, cut, head, tail, tlen))
    n = len(sidx)
    carries = zero_carries(cuda, n)
    caps = np.full(n, 2)
    w1, woff, l1 = tiny_reads(head, cut, TEXT, seed=31 + 2 * part)               # TEXT, fin = 0
    w2, _, l2 = tiny_reads(tail, tlen, 0x80 | CONT, seed=32 + 2 * part)          # CONT, fin = 1

    def name(i):
        s = c.string(int(sidx[i]))
        return f"connection {i}: [{s[:cut[i]].hex()}] then [{s[cut[i]:].hex()}]"

    def slots(rows):                                  # the parts as dst holds them: 16-byte slots, zeros behind
        out = np.zeros((len(rows), 16), dtype=np.uint8)
        out[:, :4] = rows
        return out.reshape(-1)

    m1, _, _, dst1 = run_multi(ctx, cuda, w1, woff, l1, caps, np.full(n, 16), MULTI["small"]["max_len"], carries)
    after1 = read_carries(carries).copy()
    same_bytes(dst1, slots(head), "dst after call 1")
    assert np.array_equal(m1["data_bytes"], cut)
    assert (m1["n_msgs"] == 0).all() and (m1["open_opcode"] == TEXT).all()
    # RefConn once per distinct first part (4,368 of them over the parts)
    memo = FIRST_PART_CARRY
    want_tail, want_bad = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    raw = head.tobytes()
    for i in range(n):
        first = raw[4 * i:4 * i + int(cut[i])]
        if first not in memo:
            out = RefConn().call(frame(TEXT, first, fin=0, key=0x1234567))
            memo[first] = (out["carry"]["utf8_tail"], out["carry"]["utf8_bad"])
        want_tail[i], want_bad[i] = memo[first]
    assert len(memo) <= 16 + 256 + 4096 and 0 < int(want_bad.sum()) < n
    assert (after1["open_opcode"] == TEXT).all() and np.array_equal(after1["open_bytes"], cut)
    bad = np.nonzero((after1["utf8_tail"] != want_tail) | (after1["utf8_bad"] != want_bad))[0]
    assert bad.size == 0, (f"{bad.size} carries wrong after call 1, the first: {name(bad[0])}: tail "
                           f"{int(after1['utf8_tail'][bad[0]]):08x} / {int(want_tail[bad[0]]):08x}, bad "
                           f"{int(after1['utf8_bad'][bad[0]])} / {int(want_bad[bad[0]])}")

    m2, ent2, base, dst2 = run_multi(ctx, cuda, w2, woff, l2, caps, np.full(n, 16), MULTI["small"]["max_len"], carries)
    after2 = read_carries(carries).copy()
    same_bytes(dst2, slots(tail), "dst after call 2")
    assert np.array_equal(m2["data_bytes"], tlen)
    e2 = ent2[base]
    assert (m2["n_msgs"] == 1).all() and (after2["open_opcode"] == 0).all() and (after2["n_msgs"] == 1).all()
    assert (e2["flags"] == CONTINUED).all() and np.array_equal(e2["len"], tlen) and (e2["opcode"] == TEXT).all()
    exp = c.ok[sidx]
    assert 0 < int(exp.sum()) < n
    report(e2["utf8_ok"], exp, name)

    # the sample through the carry call: nine launches per call, so 1 in 64
    pick = np.sort(np.random.default_rng(64 + part).choice(n, n // 64, replace=False))
    k = len(pick)
    single = zero_carries(cuda, k)
    for call, (w, lens, multi_m, multi_c, rows) in enumerate(((w1, l1, m1, after1, head), (w2, l2, m2, after2, tail))):
        got_m, got_e, _, got_d = run_carry_each(ctx, cuda, w.reshape(n, 16)[pick].reshape(-1).copy(), woff[:k],
                                                lens[pick], 2, np.full(k, 16), single)
        same_bytes(got_d, slots(rows[pick]), f"dst of the carry calls, call {call + 1}")
        assert read_carries(single).tobytes() == multi_c[pick].tobytes(), \
            f"call {call + 1}: the carries differ from the multi call's"
        assert got_m.tobytes() == multi_m[pick].tobytes(), f"call {call + 1}: the results differ from the multi call's"
        if call == 1:
            assert got_e[::2].tobytes() == e2[pick].tobytes(), "the entries differ from the multi call's"
            report(got_e[::2]["utf8_ok"], exp[pick], lambda j: name(int(pick[j])) + " (carry call)")


# ================================================================== C. plumbing: corpus S on the seams
# ------------------------------------------------------------------ k_utf8 / utf8_region_bad
def validate_cases(a, seqs):
    """Regions that start a bytes past a 16-B boundary. k_utf8's steps start at lo & ~15, so the
    lane seam 512 bytes and the step seam 1024 bytes behind that are at body offsets 512 - a
    and 1024 - a."""
    align = (0, CHUNK, a)
    total = STEP + 96
    return (seam_cases(total, 32 * CHUNK - a, seqs, align, "the seam of lanes 31 / 32") +
            seam_cases(total, STEP - a, seqs, align, "the 1 KiB step seam") +
            head_cases(40, seqs, align) + tail_cases(40, seqs, align) + tail_cases(STEP - a, seqs, align))


@pytest.mark.parametrize("a", [0, 13])
def test_seams_validate(ctx, cuda, a):
    """k_utf8: `prev = __shfl_up(v.w, 1)` at a lane seam in the middle of a region;
    `if (lane == 0) prev = carry` at the 1 KiB step seam (steps start at lo & ~15); sel_bytes
    at the region's first bytes with lead bytes just before lo (a leak makes a leading 80
    well-formed) and at its last bytes with continuation bytes just after hi (a leak completes
    a cut sequence), also where hi is the step seam: the `w0 < hi + 3` trip that sees only zeros."""
    cases = validate_cases(a, S)
    buf, offs, lens = place_regions(cases, seed=40 + a)
    assert (offs % CHUNK == a).all()
    check_cases(cases, run_validate(ctx, cuda, buf, offs, lens), lambda i: f"at byte {int(offs[i])}")


def test_seams_validate_every_alignment(ctx, cuda):
    """The same seams with the region start at each of 16 alignments (sel_bytes' shifts, the
    number of chunks a region meets), one well-formed and one ill-formed sequence per length."""
    cases = [c for a in range(CHUNK) for c in validate_cases(a, REPRESENTATIVES)]
    buf, offs, lens = place_regions(cases, seed=39)
    assert sorted(set((offs % CHUNK).tolist())) == list(range(CHUNK))
    check_cases(cases, run_validate(ctx, cuda, buf, offs, lens), lambda i: f"at byte {int(offs[i])}")


@pytest.mark.parametrize("call", ["messages", "carry"])
@pytest.mark.parametrize("a", [0, 13])
def test_seams_message_regions(ctx, cuda, a, call):
    """utf8_region_bad<false> as k_utf8_msgs<false> (fws_gpu_decode_messages) and k_utf8_msgs<true>
    (the carry call, a new connection) walk it: the regions of test_seams_validate as TEXT
    messages in dev_dst, so the same lane seam (`__shfl_up`), step seam (`if (lane == 0) prev =
    carry`) and first / last bytes; BIN messages of hostile bytes put every region a bytes past
    a 16-B boundary and are its neighbours in dst."""
    cases = validate_cases(a, S)
    buf, offs, lens = place_regions(cases, seed=45 + a)
    rng = np.random.default_rng(46)
    w, is_text, pos = [], [], 0
    for o, n in zip(offs.tolist(), lens.tolist()):
        if o > pos:
            w.append(frame_pair(BIN, buf[pos:o].tobytes(), 1, int(rng.integers(1, 2**32)))[0])
            is_text.append(False)
        w.append(frame_pair(TEXT, buf[o:o + n].tobytes(), 1, int(rng.integers(1, 2**32)))[0])
        is_text.append(True)
        pos = o + n
    raw, is_text = b"".join(w), np.array(is_text)
    wire = np.frombuffer(raw + bytes((-len(raw)) % 16), dtype=np.uint8).copy()
    ent, dst, nbytes = run_messages(ctx, cuda, wire, len(raw), len(w), len(w), carry=call == "carry")
    assert nbytes == pos
    same_bytes(dst[:pos], buf[:pos], "dst")
    assert np.array_equal(ent["off"][is_text], offs) and (ent["opcode"][is_text] == TEXT).all()
    assert not ent["utf8_ok"][~is_text].any(), "a BIN message was given a verdict"
    check_cases(cases, ent["utf8_ok"][is_text], lambda i: f"at dst byte {int(offs[i])}")


# ------------------------------------------------------------------ the byte-space kernels: sorted, stream
LONG = 2 * UNIT + 640            # a frame whose middle units meet no other frame (the fast kind)
SEAM_GROUPS = ("unit", "step", "lane", "ends", "unit_end", "shared_chunk")


@functools.lru_cache(maxsize=None)
def unit_cases(group):
    """Cases whose alignment is in bytes of the space the kernel walks, modulo the 4 KiB unit."""
    q = UNIT + 300
    if group == "unit":          # the seam kernels' three bytes, inside a long frame
        return seam_cases(LONG, q, S, (q, UNIT, 0), "the 4 KiB unit seam")
    if group == "step":          # the second step of a unit: lane 0's left context is lane 63's
        return seam_cases(LONG, q, S, (q, UNIT, STEP), "the 1 KiB step seam")
    if group == "lane":
        return seam_cases(LONG, q, S, (q, UNIT, STEP + 33 * CHUNK), "a 16-B lane seam")
    if group == "ends":          # short frames (several to a unit) and long ones
        return head_cases(100) + tail_cases(100) + head_cases(LONG) + tail_cases(LONG)
    if group == "unit_end":      # the frame's end at unit seam + d with s as its last bytes
        return [Case(c.body, c.ok, c.seq, c.note + f", ending at a unit seam {d:+d}", (len(c.body), UNIT, d % UNIT))
                for d in range(-3, 4) for c in tail_cases(2600)]
    assert group == "shared_chunk"
    out = []
    for i, s in enumerate(S):    # s ends one frame, another member of S starts the next in the same 16-B chunk
        for t in (S[(7 * i + 3) % len(S)], b"\x80", b"\xbf", uc.seq_v()[i % 16]):
            body, ok = uc.s_case(24, s, 0)       # its end 4 bytes into a chunk
            out.append(Case(body, ok, s, f"[{s.hex()}] ends the frame before [{t.hex()}]", (len(body), CHUNK, 4)))
            out.append(Case(*uc.s_case(0, t, 24), t, f"[{t.hex()}] starts the frame behind [{s.hex()}]", gap=0))
    return out


@functools.lru_cache(maxsize=None)
def sorted_layout(group):
    # a first region at byte 0: the units are counted from the first region's chunk, so in buffer offsets
    cases = [Case(*uc.s_case(0, S[0], 10), S[0], "the batch's first region")] + list(unit_cases(group))
    buf, offs, lens = place_regions(cases, seed=50)
    assert int(offs[0]) == 0
    if group == "shared_chunk":  # regions back to back, their seam 4 bytes into a chunk
        assert (offs[2::2] == offs[1::2] + lens[1::2]).all() and (offs[2::2] % CHUNK == 4).all()
    keys, phases = random_keys(len(cases), 51)
    return cases, buf, mask_regions(buf, offs, lens, keys, phases), offs, lens, keys, phases


@pytest.mark.parametrize("group", SEAM_GROUPS)
def test_seams_sorted(ctx, cuda, sorted_form, group):
    """fws_gpu_unmask_sorted_utf8, all three forms. unit: bytes 0..2 of a unit, which the unmask
    kernel leaves to k_utf8_seam_sorted (`utf8_err(x, p) & 0x00FFFFFF`, p the unit before's last
    dword from the seam words). step / lane: utf8_chunk_err32's left context inside a fast-kind
    unit (lane 63's last dword of the step before; the neighbour lane's). ends: sel masks at a
    frame's first and last bytes, short frames through utf8_slow_chunk. unit_end: a cut sequence
    whose error falls on the zero bytes behind the frame, in the next unit's first bytes.
    shared_chunk: two regions in one chunk, each judged with the other's bytes masked out."""
    cases, plain, masked, offs, lens, keys, phases = sorted_layout(group)
    got = run_sorted(ctx, cuda, plain, masked, offs, lens, keys, phases)
    check_cases(cases, got, lambda i: f"at byte {int(offs[i])} (unit offset {int(offs[i]) % UNIT}), form {sorted_form}")


@functools.lru_cache(maxsize=None)
def stream_layout(group):
    cases = list(unit_cases(group))   # (shared_chunk: a payload ends 4 bytes into a chunk, the next begins 6 bytes on)
    wire, plain, idx, nf, n = place_frames(cases, seed=52)
    return cases, wire, plain, idx, nf, n


@pytest.mark.parametrize("group", SEAM_GROUPS)
def test_seams_decode_stream(ctx, cuda, stream_pf, group):
    """fws_gpu_decode_stream with utf8_ok, prefetch on and off: the same seams in stream bytes
    (units are counted from the wire's first byte). unit: k_utf8_seam's three bytes; step / lane:
    the left context inside a unit of k_unmask_stream<utf8>; shared_chunk: two payloads and the
    header between them in one chunk."""
    cases, wire, plain, idx, nf, n = stream_layout(group)
    got = run_stream(ctx, cuda, wire, plain, n, nf)
    other = np.ones(nf, dtype=bool)
    other[idx] = False
    assert not got[other].any(), "a BIN frame was given a verdict"
    check_cases(cases, got[idx], lambda i: f"frame {int(idx[i])}, prefetch {stream_pf}")


# ------------------------------------------------------------------ k_utf8_msgs<false>
def test_seams_messages_fragment_split(ctx, cuda):
    """fws_gpu_decode_messages: s split between two fragments at every j -- the check sees the
    gathered bytes (k_gather_fast's region seams), never the fragments."""
    rng = np.random.default_rng(60)
    cases, w, nf = [], [], 0
    for s in S:
        for j in range(len(s) + 1):
            body, ok = uc.s_case(21, s, 22)
            cases.append(Case(body, ok, s, f"[{s.hex()}] split after byte {j}"))
            parts = (body[:21 + j], body[21 + j:])
            for f, p in enumerate(parts):
                w.append(frame_pair(CONT if f else TEXT, p, f, int(rng.integers(1, 2**32)))[0])
                nf += 1
    raw = b"".join(w)
    wire = np.frombuffer(raw + bytes((-len(raw)) % 16), dtype=np.uint8).copy()
    ent, dst, nbytes = run_messages(ctx, cuda, wire, len(raw), nf, len(cases))
    same_bytes(dst[:nbytes], np.frombuffer(b"".join(c.body for c in cases), dtype=np.uint8), "dst")
    assert (ent["n_data_frames"] == 2).all()
    check_cases(cases, ent["utf8_ok"], lambda i: f"at dst byte {int(ent['off'][i])}")


def test_seams_messages_boundary_in_a_chunk(ctx, cuda):
    """A message boundary inside one 16-B chunk of dev_dst: the message before ends with a cut
    sequence (a member of P), the next begins with 80 / BF -- both ill-formed, though together
    they would read as one character -- or with a member of V, which stays well-formed
    (utf8_region_bad's sel_bytes on both sides of hi / lo in one chunk)."""
    rng = np.random.default_rng(61)
    cases, w, pos = [], [], 0
    for p in uc.seq_p():
        for t in (b"\x80", b"\xbf") + uc.seq_v():
            before = 20 + (5 - (pos + 20 + len(p))) % CHUNK          # the boundary 5 bytes into a chunk
            a = Case(*uc.s_case(before, p, 0), p, f"[{p.hex()}] ends the message before [{t.hex()}]")
            b = Case(*uc.s_case(0, t, 20), t, f"[{t.hex()}] begins the message behind [{p.hex()}]")
            pos += len(a.body)
            assert pos % CHUNK == 5
            pos += len(b.body)
            cases += [a, b]
            w += [frame_pair(TEXT, c.body, 1, int(rng.integers(1, 2**32)))[0] for c in (a, b)]
    raw = b"".join(w)
    wire = np.frombuffer(raw + bytes((-len(raw)) % 16), dtype=np.uint8).copy()
    ent, dst, nbytes = run_messages(ctx, cuda, wire, len(raw), len(cases), len(cases))
    same_bytes(dst[:nbytes], np.frombuffer(b"".join(c.body for c in cases), dtype=np.uint8), "dst")
    assert not any(c.ok for c in cases[::2])
    check_cases(cases, ent["utf8_ok"], lambda i: f"at dst byte {int(ent['off'][i])}")


# ------------------------------------------------------------------ the open part: prefix mode, the tail, the seed
@functools.lru_cache(maxsize=None)
def call_boundary_cases(part):
    """(cases, call 1's reads, call 2's reads, RefConn's utf8_tail / utf8_bad / open_bytes after call 1,
    the cuts). The (s, j) cases are dealt over PARTS test cases; each meets one of the 16 end phases."""
    cases, w1, w2, want, cuts, k = [], [], [], [], [], -1
    rng = np.random.default_rng(80)
    for s in S:
        for j in range(len(s) + 1):
            k += 1
            if k % PARTS != part:
                continue
            cut = STEP + 21 + k // PARTS % CHUNK
            body, ok = uc.s_case(cut - j, s, 30)
            cases.append(Case(body, ok, s, f"[{s.hex()}] cut after byte {j}, parts of {cut} and {len(body) - cut} bytes"))
            w1.append(frame_pair(TEXT, body[:cut], 0, int(rng.integers(1, 2**32)))[0])
            w2.append(frame_pair(CONT, body[cut:], 1, int(rng.integers(1, 2**32)))[0])
            ref = RefConn().call(frame(TEXT, body[:cut], fin=0, key=0))["carry"]
            want.append((ref["utf8_tail"], ref["utf8_bad"], ref["open_bytes"]))
            cuts.append(cut)
    return cases, w1, w2, np.array(want, dtype=np.int64), cuts


@pytest.mark.parametrize("part", range(PARTS))
@pytest.mark.parametrize("call", ["multi", "carry"])
def test_seams_call_boundary(ctx, cuda, call, part):
    """s cut between two calls at every j, the first part longer than a wave step and ending
    at each byte of a chunk in turn (a sample: each (s, j) meets one of the 16 end phases). Call 1 (TEXT fin=0): the open part judged in prefix mode
    -- utf8_region_bad<true> / kMmPrefix count an error only at the part's own bytes
    (`utf8_err(...) & sx`, every dword of the chunk), a cut sequence is no error yet -- and the
    tail rebuilt from its last 3 bytes; both must be RefConn's. Call 2 (CONT fin=1): the seeded
    region (old_tail as the left context of dst byte 0, the sticky error); Python's verdict."""
    cases, w1, w2, want, cuts = call_boundary_cases(part)
    n = len(cases)
    assert 0 < int(want[:, 1].sum()) < n
    carries = zero_carries(cuda, n)

    def launch(wires, plains, what):
        """the reads through the call under test; the part each delivers must be in its dst"""
        host, woff, lens = lay_reads(wires)
        if call == "carry":
            out = run_carry_each(ctx, cuda, host, woff, lens, 2, lens, carries)
        else:
            out = run_multi(ctx, cuda, host, woff, lens, np.full(n, 2), lens, MULTI["small"]["max_len"], carries)
        check_dst(out[3], woff, plains, what)
        assert np.array_equal(out[0]["data_bytes"], [len(p) for p in plains])
        return out

    m, _, _, _ = launch(w1, [c.body[:q] for c, q in zip(cases, cuts)], "dst after call 1")
    got = read_carries(carries)
    assert (m["n_msgs"] == 0).all() and (got["open_opcode"] == TEXT).all()
    bad = np.nonzero((got["utf8_tail"] != want[:, 0]) | (got["utf8_bad"] != want[:, 1]) | (got["open_bytes"] != want[:, 2]))[0]
    assert bad.size == 0, (f"{bad.size} carries wrong after call 1, the first: {cases[bad[0]].note}: tail "
                           f"{int(got['utf8_tail'][bad[0]]):08x} / {int(want[bad[0], 0]):08x}, bad "
                           f"{int(got['utf8_bad'][bad[0]])} / {int(want[bad[0], 1])}")
    m, ent, base, _ = launch(w2, [c.body[q:] for c, q in zip(cases, cuts)], "dst after call 2")
    e = ent[base]
    assert (m["n_msgs"] == 1).all() and (e["flags"] == CONTINUED).all() and (read_carries(carries)["open_opcode"] == 0).all()
    check_cases(cases, e["utf8_ok"], lambda i: f"connection {i}, {call} call")


# ------------------------------------------------------------------ k_msg_multi
def multi_seams(form, kind):
    """Byte positions, in a read's dst space, of the chunk seams of k_msg_multi: a wave takes
    steps * 64 consecutive chunks, steps = ceil(((db + 18) >> 4) / threads)."""
    f = MULTI[form]
    nck = (f["read"] + 18) >> 4
    steps = -(-nck // f["threads"])
    waves = f["threads"] // LANES
    assert steps > 1 and f["read"] <= f["max_len"] - 32
    if kind == "wave":           # each wave's first chunk: its left context is assembled once more (st == 0)
        chunks = [w * steps * LANES for w in range(1, waves)]
    elif kind == "step":         # lane 0 of a later step: the carry from lane 63
        chunks = [(w * steps + st) * LANES for w in range(waves) for st in range(1, steps)]
    else:                        # a lane seam: the neighbour's last dword by __shfl_up
        chunks = [(w * steps + st) * LANES + 37 for w in range(waves) for st in range(steps)]
    chunks = [c for c in chunks if 2 <= c < nck - 3]     # (the last waves of the full form have no chunk)
    assert len(chunks) >= 3
    return [CHUNK * c for c in chunks]


@pytest.mark.parametrize("part", range(PARTS))
@pytest.mark.parametrize("variant", ["whole", "split", "continued"])
@pytest.mark.parametrize("kind", ["lane", "step", "wave"])
@pytest.mark.parametrize("form", list(MULTI))
def test_seams_multi(ctx, cuda, form, kind, variant, part):
    """fws_gpu_decode_messages_multi, one read per case, its TEXT message's bytes filling the
    read's dst space with s across a seam of the walk. The (s, j) cases are dealt over PARTS
    test cases and, within one, over the seams of the kind in turn: a sample per seam (every
    wave's first chunk is met by some of S, and by the filler's characters in every read). In
    the small form every (s, j) also runs on the first seam of its kind, so all of S meets one
    seam of each kind. lane: `prev = __shfl_up(v.w, 1)`; step: `if (wlane == 0) prev = carry`; wave: the
    `st == 0` re-assembly of the chunk before a wave's first. split: the message in two
    fragments that meet at the seam (dst_chunk gathers the chunk from both frames); continued:
    the same, the message opened by an earlier call (a seeded region: kMmSeeded, old_tail)."""
    f = MULTI[form]
    total, seams = f["read"], multi_seams(form, kind)
    rng = np.random.default_rng(70)
    opener = uc.filler(27, "right")
    cases, w1, w2, k = [], [], [], -1
    for s in S:
        for j in range(len(s) + 1):
            k += 1
            if k % PARTS != part:
                continue
            dealt = seams[k // PARTS % len(seams)]
            for q in dict.fromkeys([dealt, seams[0]] if form == "small" else [dealt]):
                body, ok = uc.s_case(q - j, s, total - (q - j) - len(s))
                cases.append(Case(body, ok, s, f"[{s.hex()}] byte {j} first past dst byte {q} (chunk {q // CHUNK})"))
                key = lambda: int(rng.integers(1, 2**32))
                if variant == "whole":
                    w2.append(frame_pair(TEXT, body, 1, key())[0])
                else:
                    first = CONT if variant == "continued" else TEXT
                    w2.append(frame_pair(first, body[:q], 0, key())[0] + frame_pair(CONT, body[q:], 1, key())[0])
                w1.append(frame_pair(TEXT, opener, 0, key())[0])
    n = len(cases)
    carries = zero_carries(cuda, n)

    def launch(wires, dst_caps, plains, what):
        host, woff, lens = lay_reads(wires)
        out = run_multi(ctx, cuda, host, woff, lens, np.full(n, 4), dst_caps, f["max_len"], carries)
        check_dst(out[3], woff, plains, what)          # every read's bytes, and nothing beside them
        return out

    if variant == "continued":
        m, _, _, _ = launch(w1, np.full(n, 32), [opener] * n, "dst after the opening call")
        assert (m["open_opcode"] == TEXT).all() and (m["n_msgs"] == 0).all()
    m, ent, base, _ = launch(w2, np.full(n, total), [c.body for c in cases], f"dst, {form} form, {variant}")
    assert (m["n_msgs"] == 1).all() and (m["data_bytes"] == total).all() and (m["open_opcode"] == 0).all()
    e = ent[base]
    assert (e["len"] == total).all() and (e["flags"] == (CONTINUED if variant == "continued" else 0)).all()
    check_cases(cases, e["utf8_ok"], lambda i: f"read {i}, {form} form, {variant}")
