"""GPU parity of the unmask and stream-decode kernels' grid-stride loops.

Every streaming kernel of the receive path gives one wavefront a 4 KiB unit
and then strides by the grid's wave count; the launchers size the grid so that
no wave takes a second turn below 256 MiB (k_mask_single, k_unmask_desc) or
16 GiB (k_unmask_sorted*, k_unmask_sorted_utf8, k_unmask_stream). Here
fws_internal_set_grid_cap(G) caps every such grid at G workgroups (4 waves
each), so buffers of 300 KiB - 4 MiB put every wave through its loop two to
six times, with trip counts that differ between the waves: the state a wave
carries from one unit to the next (k_unmask_stream's cross-unit prefetch,
k_unmask_desc's record prefetch, the software-pipelined sorted UTF-8 form),
the owner guess of a later unit and the XCD-run workgroup map on a grid whose
last group of 64 is partial are all run and compared.

Every comparison is bit-exact against the oracle (tests/orc.py: the
restatement of WSMaskBytesFast and of OnRecvData / ParseFrameHdr), UTF-8 flags
against Python's strict decoder; whole buffers are compared, so bytes outside
the payloads are checked too.

Not here: fws_gpu_unmask_batch's opt-in k_unmask_any form (its grids are not
under the cap hook; test_gpu_unmask.py's test_any_* run it with striding waves)
and k_utf8_seam_sorted's own cap of 4096 workgroups (1 Mi units; it strides in
test_gpu_configs.py's 4 GiB share).
"""
import functools
import struct

import numpy as np
import pytest
import torch

import orc
from flashws_amd import _lib, gpu

pytestmark = pytest.mark.gpu

WAVES = 4                      # kBlock / kWave: wavefronts (units in flight) per workgroup
# workgroup caps: 4 waves; 12 (no power of two); 256 = one full XCD-run group of 64 workgroups;
# 400 = one full group and a partial one of 36 (the case xcd_run_block's guard is for)
CAPS = [1, 3, 64, 100]
SMALL, BIG = 307_000, 4_200_000          # bytes of span for G in {1, 3} / {64, 100}


def span_for(G):
    return SMALL if G <= 3 else BIG


# ---------------------------------------------------------------- hooks
HOOK_DEFAULTS = {"grid_cap": 0, "unmask_any": 0, "sorted_early": 0, "sorted_utf8_pipe": 2, "stream_variant": 0,
                 "stream_utf8_pf": 1}


class Hooks:
    """Process-global tuning hooks set for one test; restore() puts every one back."""

    def __init__(self):
        self.saved = []

    def set(self, name, value):
        assert name in HOOK_DEFAULTS
        old = getattr(_lib.lib(), "fws_internal_set_" + name)(int(value))
        self.saved.append((name, old))

    def restore(self):
        while self.saved:
            name, old = self.saved.pop()
            getattr(_lib.lib(), "fws_internal_set_" + name)(old)


@pytest.fixture
def hooks():
    h = Hooks()
    try:
        yield h
    finally:
        h.restore()


# ---------------------------------------------------------------- unit counts (host arithmetic)
def chunks_of(addr, n):
    """fws_device.h chunks_of: 16-B chunks meeting [addr, addr + n)."""
    return 0 if n == 0 else ((addr + n + 15) >> 4) - (addr >> 4)


def span_units(descs, shift=0):
    """Units of the byte-space loops (k_unmask_desc in byte space, unmask_sorted_body): 4 KiB units from
    the 16-B boundary at or below the first payload byte to the last one; shift = base address mod 16."""
    sa = (shift + int(descs["payload_off"][0])) & ~15
    e1 = shift + int(descs["payload_off"][-1]) + int(descs["payload_len"][-1])
    return (e1 - sa + 4095) // 4096 if e1 > sa else 0


def chunk_units(descs):
    """Units of k_unmask_desc's chunk-space loop (a 16-B aligned base): 256 chunks each."""
    po, ln = descs["payload_off"].astype(np.int64), descs["payload_len"].astype(np.int64)
    total = int(np.where(ln > 0, ((po + ln + 15) >> 4) - (po >> 4), 0).sum())
    return (total + 255) // 256


def assert_strides(what, G, units):
    """Every wave of the capped grid iterates at least twice and the waves' trip counts differ."""
    nwaves = WAVES * G
    print(f"{what}: cap {G} = {nwaves} waves, {units} units")
    assert units > 2 * nwaves, (what, G, units)
    assert units % nwaves != 0, (what, G, units)


def strides_at_every_cap(units, span):
    return all(units > 2 * WAVES * G and units % (WAVES * G) != 0 for G in CAPS if span_for(G) == span)


def first_that_strides(build, units_of, span):
    """build(span + a few KiB): the first result whose unit count meets assert_strides at every cap
    that uses this span (random lengths decide the exact size of a shape)."""
    for bump in range(32):
        shape = build(span + 4096 * bump)
        if strides_at_every_cap(units_of(shape), span):
            return shape
    raise AssertionError("no size near the span meets the unit rule")


# ---------------------------------------------------------------- descriptor shapes
MIXED_LENS = [0, 1, 5, 125, 126, 700, 3000, 9000, 70000]


def _descs(rng, lens, gaps, start):
    lens, gaps = np.asarray(lens, dtype=np.int64), np.asarray(gaps, dtype=np.int64)
    step = lens + gaps
    offs = start + np.concatenate([[0], np.cumsum(step[:-1])])
    d = np.zeros(len(lens), dtype=gpu.FRAME_DESC)
    d["payload_off"], d["payload_len"] = offs, lens
    d["key"] = rng.integers(0, 2**32, len(lens), dtype=np.uint64).astype(np.uint32)
    d["phase"] = rng.integers(0, 4, len(lens))
    return d, int(offs[-1] + lens[-1])


def _cut_to_span(lens, gaps, span):
    k = int(np.searchsorted(np.cumsum(lens + gaps), span)) + 1
    assert k < len(lens)
    return lens[:k], gaps[:k]


def oracle_regions(buf, descs):
    """The oracle's WSMaskBytesFast on every region of a copy of buf (phase = the key rotated)."""
    out = buf.copy()
    L = orc.orc()
    mask, rot, p = L.orc_ws_mask_fast, L.orc_rotr32, out.ctypes.data
    for o, n, k, ph in zip(descs["payload_off"].tolist(), descs["payload_len"].tolist(), descs["key"].tolist(),
                           descs["phase"].tolist()):
        if n:
            mask(p + o, n, rot(k, 8 * ph))
    return out


def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


@functools.lru_cache(maxsize=None)
def desc_shape(name, span):
    """(host bytes, sorted descriptors, oracle result) of a shape; built once, never written.
    Every shape starts at an offset that is not 16-B aligned."""
    rng = np.random.default_rng([span, sum(map(ord, name))])
    if name == "mixed":                  # fast, slow and shared-chunk units in one batch
        lens = rng.choice(MIXED_LENS, 4096).astype(np.int64)
        lens, gaps = _cut_to_span(lens, rng.integers(0, 21, 4096), span)
        descs, end = _descs(rng, lens, gaps, 5)
    elif name == "tiny":                 # far more than 64 regions per unit: slow-kind units throughout
        n = span // 16
        lens, gaps = _cut_to_span(rng.integers(0, 40, n), rng.integers(0, 4, n), span)
        descs, end = _descs(rng, lens, gaps, 3)
    elif name == "sparse":               # 64 B every 1 MiB: most units hold no payload
        n = 2 if span == SMALL else 5
        descs, end = _descs(rng, [64] * n, [(1 << 20) - 64] * n, 3)
    elif name == "sparse_near":          # 64 B every 512 B: sorted, yet too sparse for byte space
        n = span // 20 + 40
        descs, end = _descs(rng, [64] * n, [448] * n, 3)
    elif name == "one_large":            # runs of one-key units
        descs, end = _descs(rng, [span], [0], 5)
    else:
        raise KeyError(name)
    host = rng.integers(0, 256, end + 64, dtype=np.uint8)
    return _frozen(host, descs, oracle_regions(host, descs))


def descs_on(descs, cuda):
    """The descriptors on the device (a copy: the cached shapes are read-only)."""
    return gpu.descs_to_device(np.array(descs), cuda)


def upload(host, cuda, shift=0):
    """host on the device behind `shift` zero bytes: (whole tensor, the view at the shifted base)."""
    dev = torch.from_numpy(np.concatenate([np.zeros(shift, np.uint8), host])).to(cuda)
    assert dev.data_ptr() % 16 == 0      # the unit counts above assume it
    return dev, dev[shift:]


# ---------------------------------------------------------------- fws_gpu_mask
@pytest.mark.parametrize("off", [0, 5, 15])
@pytest.mark.parametrize("G", CAPS)
def test_mask_capped(cuda, hooks, G, off):
    """k_mask_single: one region of 1 B, 5 units + 3 B and the whole span at offsets 0, 5 and 15."""
    span = span_for(G)
    host = np.random.default_rng(G * 16 + off).integers(0, 256, span + 64, dtype=np.uint8)
    hooks.set("grid_cap", G)
    for n in (1, 4096 * 5 + 3, span):
        if n == span:
            assert_strides(f"mask off {off}", G, (chunks_of(off, n) + 255) // 256)
        key = 0x9E3779B1 * (n + off + 1) & 0xFFFFFFFF
        dev, _ = upload(host, cuda)
        gpu.ws_mask_bytes_fast(dev, key, off, n)
        exp = host.copy()
        orc.orc_mask("ws_mask_fast", exp, key, off, n)
        assert np.array_equal(dev.cpu().numpy(), exp), (G, off, n)


# ---------------------------------------------------------------- fws_gpu_unmask_batch, planned
# (shape, permuted, byte space expected)
PLANNED = [("mixed", False, 1), ("mixed", True, 0), ("tiny", False, 1), ("tiny", True, 0), ("one_large", False, 1),
           ("sparse", False, 0), ("sparse", True, 0), ("sparse_near", False, 0), ("sparse_near", True, 0)]


@pytest.mark.parametrize("shape,permute,byte_space", PLANNED,
                         ids=[f"{s}-{'permuted' if p else 'sorted'}" for s, p, _ in PLANNED])
@pytest.mark.parametrize("G", CAPS)
def test_unmask_batch_planned_capped(ctx, cuda, hooks, G, shape, permute, byte_space):
    """k_plan + k_unmask_desc: sorted batches in byte space (the record prefetch unit_rec[u + nwaves]),
    permuted and sparse ones in chunk space. A one-region batch has no second order. The sparse
    shape at 1 MiB steps has a handful of chunk-space units at any buffer size a test can afford, so
    the striding sparse case of the chunk-space loop is sparse_near."""
    host, descs, exp = desc_shape(shape, span_for(G))
    if permute:
        descs = descs[np.random.default_rng(G).permutation(len(descs))]
    if shape != "sparse":
        assert_strides(f"planned {shape} {'chunk' if not byte_space else 'byte'} space", G,
                       span_units(descs) if byte_space else chunk_units(descs))
    hooks.set("unmask_any", 0)
    hooks.set("grid_cap", G)
    dev, base = upload(host, cuda)
    gpu.unmask_batch(ctx, base, descs_on(descs, cuda), len(descs))
    got = dev.cpu().numpy()
    assert gpu.plan_mode(ctx)["byte_space"] == byte_space
    assert np.array_equal(got, exp)


# ---------------------------------------------------------------- fws_gpu_unmask_sorted
SORTED = [("mixed", 0), ("tiny", 0), ("sparse", 0), ("one_large", 0), ("mixed", 1), ("mixed", 15)]


@pytest.mark.parametrize("shape,shift", SORTED, ids=[f"{s}-shift{k}" for s, k in SORTED])
@pytest.mark.parametrize("form", [0, 1, 3], ids=["lookup_first", "early", "xcd_runs"])
@pytest.mark.parametrize("G", CAPS)
def test_unmask_sorted_capped(ctx, cuda, hooks, G, form, shape, shift):
    """unmask_sorted_body past a wave's first unit: the owner guess of unit u + k * nwaves, gap units
    skipped between real ones, and the XCD-run workgroup order on full and partial groups of 64."""
    host, descs, exp = desc_shape(shape, span_for(G))
    assert_strides(f"sorted {shape} shift {shift}", G, span_units(descs, shift))
    hooks.set("sorted_early", form)
    hooks.set("grid_cap", G)
    dev, base = upload(host, cuda, shift)
    gpu.unmask_sorted(ctx, base, descs_on(descs, cuda), len(descs))
    got = dev.cpu().numpy()
    assert not got[:shift].any()
    assert np.array_equal(got[shift:], exp)


# ---------------------------------------------------------------- text
@functools.lru_cache(maxsize=None)
def text_pool():
    """Valid UTF-8 of 1-4-byte characters and the byte offset of every character."""
    rng = np.random.default_rng(1234)
    cps = np.concatenate([rng.integers(0x20, 0x7F, 30000), rng.integers(0x80, 0x800, 20000),
                          rng.integers(0x800, 0xD800, 20000), rng.integers(0x10000, 0x110000, 20000)])
    rng.shuffle(cps)
    enc = [chr(int(c)).encode() for c in cps]
    starts = np.concatenate([[0], np.cumsum([len(e) for e in enc])])
    return b"".join(enc), starts


def text(rng, n):
    """About n bytes of whole characters (at most 3 short per 64 KiB)."""
    pool, starts = text_pool()
    out = []
    while n > 0:
        m = min(n, 65536)
        i = int(rng.integers(0, len(starts) - 1 - m))     # every character is at least one byte
        j = int(np.searchsorted(starts, starts[i] + m, side="right")) - 1
        out.append(pool[starts[i]:starts[j]])
        n -= m
    return b"".join(out)


PATCHES = [b"\xff", b"\xe2\x82a", b"\xc0", b"\xf0\x9f"]      # invalid bytes, cut sequences


def valid(b):
    try:
        bytes(b).decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


@functools.lru_cache(maxsize=None)
def text_shape(name, span, shift):
    return first_that_strides(lambda size: _text_shape(name, size, shift), lambda t: span_units(t[1], shift), span)


def _text_shape(name, span, shift):
    """(masked host bytes, descriptors, oracle result, expected flags): text regions 0-20 arbitrary
    high bytes apart, about 5 % of them corrupted -- an invalid byte or a cut sequence anywhere, a
    sequence cut by the region's end, or either in the first three bytes of a 4 KiB unit of the span
    or the last three of the unit before it (unit boundaries: (base + first offset) & ~15 plus a
    multiple of 4096; shift = base mod 16)."""
    rng = np.random.default_rng([span, shift, len(name)])
    lo, hi = (4096, 40960) if name == "long" else (0, 200)
    bodies, total = [], 0
    while total < span:
        bodies.append(bytearray(text(rng, int(rng.integers(lo, hi + 1)))))
        total += len(bodies[-1]) + 10
    n = len(bodies)
    n_bad = max(4, n // 20)
    for r in rng.integers(0, n, (n_bad + 3) // 4):        # a sequence cut by the region's end
        bodies[int(r)] += b"\xe2\x82"
    start = 7
    descs, end = _descs(rng, [len(b) for b in bodies], rng.integers(0, 21, n), start)
    offs = descs["payload_off"].astype(np.int64)
    first_unit = ((shift + start) & ~15) - shift          # base-relative offset of unit 0
    n_units = (end - first_unit + 4095) // 4096
    for k in range(n_bad - (n_bad + 3) // 4):
        patch = PATCHES[k % len(PATCHES)]
        if k % 3 < 2:                                     # at a unit boundary: its first three / last three bytes
            at = first_unit + 4096 * int(rng.integers(1, n_units)) + (k // 3 % 3 if k % 3 == 0 else -1 - k // 3 % 3)
            r = int(np.searchsorted(offs, at, side="right")) - 1
        else:                                             # anywhere
            r = int(rng.integers(0, n))
            at = int(offs[r]) + int(rng.integers(0, len(bodies[r]) + 1))
        if r < 0 or at < offs[r] or at + len(patch) > offs[r] + len(bodies[r]):
            continue                                      # (the boundary lies in a gap, or the patch does not fit)
        bodies[r][at - int(offs[r]):at - int(offs[r]) + len(patch)] = patch
    plain = rng.integers(0x80, 0x100, end + 64, dtype=np.uint8)
    for o, b in zip(descs["payload_off"].tolist(), bodies):
        plain[o:o + len(b)] = np.frombuffer(bytes(b), dtype=np.uint8)
    flags = np.array([valid(b) for b in bodies])
    assert 0 < (~flags).sum() < n
    masked = oracle_regions(plain, descs)                 # (the XOR is an involution)
    return _frozen(masked, descs, oracle_regions(masked, descs), flags)


@pytest.mark.parametrize("shape,shift", [("long", 0), ("short", 0), ("long", 9)])
@pytest.mark.parametrize("form", [0, 1, 2], ids=["plain", "pipe", "early"])
@pytest.mark.parametrize("G", CAPS)
def test_unmask_sorted_utf8_capped(ctx, cuda, hooks, G, form, shape, shift):
    """k_unmask_sorted_utf8's three forms: the seam words of a wave's later units, the pipelined
    form's carried lookup and loads, errors at unit boundaries two strides apart."""
    masked, descs, exp, flags = text_shape(shape, span_for(G), shift)
    assert_strides(f"sorted_utf8 {shape} shift {shift}", G, span_units(descs, shift))
    hooks.set("sorted_utf8_pipe", form)
    hooks.set("grid_cap", G)
    dev, base = upload(masked, cuda, shift)
    ok = torch.full((len(descs),), 7, dtype=torch.uint8, device=cuda)
    gpu.unmask_sorted_utf8(ctx, base, descs_on(descs, cuda), len(descs), ok)
    got = dev.cpu().numpy()
    assert not got[:shift].any()
    assert np.array_equal(got[shift:], exp)
    okh = ok.cpu().numpy()
    assert set(np.unique(okh)) <= {0, 1}
    assert np.array_equal(okh.astype(bool), flags), np.flatnonzero(okh.astype(bool) != flags)[:10]


# ---------------------------------------------------------------- fws_gpu_decode_stream
def build_wire(frames):
    """Client frames back to back: frames = [(opcode, fin, payload bytes, key, len_form or None)]."""
    parts, pay_off, pos = [], [], 0
    for op, fin, body, key, form in frames:
        n = len(body)
        form = form if form else (n if n < 126 else (126 if n <= 65535 else 127))
        h = bytes([(fin << 7) | op])
        if form == 126:
            h += bytes([0x80 | 126]) + struct.pack(">H", n)
        elif form == 127:
            h += bytes([0x80 | 127]) + struct.pack(">Q", n)
        else:
            h += bytes([0x80 | n])
        h += struct.pack("<I", key)
        parts += [h, bytes(body)]
        pay_off.append(pos + len(h))
        pos += len(h) + n
    wire = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
    lens = np.array([len(f[2]) for f in frames], dtype=np.int64)
    kb = np.array([f[3] for f in frames], dtype="<u4").view(np.uint8).reshape(-1, 4)
    k = np.arange(int(lens.sum())) - np.repeat(np.cumsum(lens) - lens, lens)
    wire[np.repeat(np.array(pay_off, dtype=np.int64), lens) + k] ^= kb[np.repeat(np.arange(len(frames)), lens), k & 3]
    return wire


def _body(rng, op, n):
    return text(rng, n) if op == 1 and n >= 4 else rng.integers(0, 256, n, dtype=np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def stream_shape(name, span):
    return first_that_strides(lambda size: _stream_shape(name, size), lambda t: (len(t[0]) + 4095) // 4096, span)


def _stream_shape(name, span):
    """(wire, oracle bytes, oracle frames, oracle status, consumed, expected flags) of a wire stream."""
    rng = np.random.default_rng([span, sum(map(ord, name))])
    frames, total = [], 0

    def add(op, fin, body, form=None):
        nonlocal total
        frames.append((op, fin, body, int(rng.integers(0, 2**32)), form))
        total += len(body) + 8
    tail = b""
    if name == "mixed":                  # BIN and TEXT, FIN 0 and 1, the three length forms
        while total < span:
            n = int(rng.choice(MIXED_LENS))
            op = int(rng.choice([1, 2]))
            form = None if rng.random() < 0.6 else (127 if n > 65535 or rng.random() < 0.5 else 126)
            body = bytearray(_body(rng, op, n))
            if op == 1 and len(body) > 8 and rng.random() < 0.2:
                body[int(rng.integers(0, len(body)))] = 0xFF
            add(op, int(rng.random() < 0.8), bytes(body), form)
        add(2, 1, rng.integers(0, 256, 9000, dtype=np.uint8).tobytes())
        cut = 777                        # the stream ends inside the last payload
    elif name == "tiny":                 # over 64 frames in every unit: the per-chunk search
        while total < span:
            op = int(rng.choice([1, 2]))
            add(op, int(rng.random() < 0.8), _body(rng, op, int(rng.integers(0, 40))))
        cut = 0
        tail = bytes([0x82, 0xFE, 0x01])  # the stream ends inside a header
    elif name == "dense":                # 3..64 frames in every unit: the lane-resident frames of the plain form
        while total < span:
            op = int(rng.choice([1, 2]))
            add(op, int(rng.random() < 0.8), _body(rng, op, int(rng.integers(40, 400))))
        cut = 0
    elif name == "text16k":              # 16 KiB TEXT frames, errors around the 4 KiB stream offsets
        pos, k = 0, 0
        while total < span:
            body = bytearray(text(rng, 16384))
            if len(frames) % 3 == 1:
                d = (0, 1, 2, -1, -2, -3)[k % 6]
                patch = PATCHES[k % len(PATCHES)]
                at = (pos + 8 + 4095) // 4096 * 4096 + 4096 * int(rng.integers(0, 3)) + d - (pos + 8)
                at += 4096 if at < 0 else 0
                body[at:at + len(patch)] = patch
                k += 1
            add(1, 1, bytes(body), 126)
            pos += 8 + len(body)
        cut = 0
    elif name == "one_large":            # one TEXT frame: one-key units, the prefetch's steady state
        add(1, 1, text(rng, span), 127)
        cut = 0
    else:
        raise KeyError(name)
    wire = build_wire(frames)
    wire = np.concatenate([wire[:len(wire) - cut], np.frombuffer(tail, dtype=np.uint8)])
    exp = wire.copy()
    ret, oframes, _, consumed = orc.orc_decode_stream(exp)
    assert ret == 0 and len(oframes) == len(frames)
    assert len(wire) > 128 * 1024 or len(frames) > 256          # never the small-read kernel's size
    flags = np.array([op == 1 and fin == 1 and valid(body) for op, fin, body, _, _ in frames])
    if cut:
        flags[-1] = False                # an incomplete frame is not judged
    return _frozen(wire, exp, oframes, flags) + (ret, consumed)


FLAG_MODES = {"no_flags": None, "flags_pf": 1, "flags_no_pf": 0}


@pytest.mark.parametrize("flag_mode", list(FLAG_MODES))
@pytest.mark.parametrize("variant", [0, 1, 2, 3], ids=["fwd_nt", "rev_nt", "fwd", "rev"])
@pytest.mark.parametrize("shape", ["mixed", "tiny", "dense", "text16k", "one_large"])
@pytest.mark.parametrize("G", CAPS)
def test_decode_stream_capped(ctx, cuda, hooks, G, shape, variant, flag_mode):
    """k_unmask_stream in its four orders / cache policies, plain and with UTF-8 flags (with and
    without the cross-unit prefetch, whose in-loop load only acts past a wave's first unit): status,
    frame count, consumed, the frame list, the whole stream (headers and unread bytes included)
    and the flags."""
    wire, exp, oframes, flags, ret, consumed = stream_shape(shape, span_for(G))
    assert_strides(f"stream {shape}", G, (len(wire) + 4095) // 4096)
    hooks.set("stream_variant", variant)
    pf = FLAG_MODES[flag_mode]
    if pf is not None:
        hooks.set("stream_utf8_pf", pf)
    hooks.set("grid_cap", G)
    dev, _ = upload(wire, cuda)
    n = len(oframes)
    ok = torch.full((n + 4,), 7, dtype=torch.uint8, device=cuda) if pf is not None else None
    rc, fr, res, _ = gpu.decode_stream(ctx, dev, cap=n + 16, utf8_ok=ok)
    assert rc == 0
    r = gpu.read_result(res)
    assert int(r["status"]) == ret
    assert int(r["n_frames"]) == n
    assert int(r["consumed"]) == consumed
    got = gpu.read_frames(fr, n)
    for k in ("hdr_off", "payload_len", "key", "opcode", "fin", "hdr_len"):
        assert np.array_equal(got[k], oframes[k]), k
    assert np.array_equal(dev.cpu().numpy(), exp)
    if ok is not None:
        okh = ok.cpu().numpy()[:n]
        assert set(np.unique(okh)) <= {0, 1}
        assert np.array_equal(okh.astype(bool), flags), np.flatnonzero(okh.astype(bool) != flags)[:10]
    c = gpu.decode_counters(ctx)         # the parallel decode ran, and resolved on the device
    assert c["frames"] == n and not c["failed"]


# ---------------------------------------------------------------- last: nothing left set
def test_zz_hooks_are_back_at_their_defaults():
    """Runs last in this file: every hook the tests above set is at its default again (each setter
    returns the previous value; the value written is the default itself)."""
    L = _lib.lib()
    for name, default in HOOK_DEFAULTS.items():
        assert getattr(L, "fws_internal_set_" + name)(default) == default, name
