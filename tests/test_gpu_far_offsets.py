"""GPU parity at byte offsets at and past 2^32.

Every descriptor field and stream length of the ABI is 64-bit; a truncating
cast in a kernel's address arithmetic shows only when an offset does not fit
32 bits. One device buffer of 4 GiB + 2 MiB (zeros) carries random bytes in
two windows, [0, 1 MiB) and [2^32 - 1 MiB, 2^32 + 2 MiB), and regions in both:
small ones, one of 100 000 B across the 2^32 line and one of 70 000 B wholly
above it. fws_gpu_unmask_batch (planned in chunk space and in byte space, and
the k_unmask_any + k_unmask_pieces form), fws_gpu_unmask_sorted,
fws_gpu_unmask_gather, fws_gpu_validate_utf8 and fws_gpu_mask run on it, each
compared bit-exact with the oracle (tests/orc.py) applied to host copies of
the two windows; after every call the 4 GiB between the windows must still be
zero (checked on the device).
"""
import numpy as np
import pytest
import torch

import orc
from flashws_amd import _lib, gpu
from test_gpu_grid_stride import _descs, descs_on, hooks, oracle_regions, text, valid  # noqa: F401 (hooks: a fixture)

pytestmark = pytest.mark.gpu

MIB = 1 << 20
LINE = 1 << 32
HI0 = LINE - MIB                         # the high window: [HI0, SIZE)
SIZE = LINE + 2 * MIB


class Far:
    """The shared buffer, its two windows' host bytes and the regions."""

    def __init__(self, cuda):
        rng = np.random.default_rng(2 ** 32 % 1000003)
        self.lo = rng.integers(0, 256, MIB, dtype=np.uint8)
        self.hi = rng.integers(0, 256, SIZE - HI0, dtype=np.uint8)
        self.buf = torch.zeros(SIZE, dtype=torch.uint8, device=cuda)
        assert self.buf.data_ptr() % 16 == 0

        def small(start, end):           # regions of 0-600 B, 0-20 B apart, in [start, end)
            n = (end - start) // 200
            lens, gaps = rng.integers(0, 601, n), rng.integers(0, 21, n)
            k = int(np.searchsorted(np.cumsum(lens + gaps), end - start - 700))
            return _descs(rng, lens[:k], gaps[:k], start)[0]

        def one(off, n):
            return _descs(rng, [n], [0], off)[0]
        parts = [small(5, MIB - 64), small(HI0 + 3, LINE - 50_000), one(LINE - 50_000, 100_000),
                 small(LINE + 50_007, LINE + MIB), one(LINE + MIB + 11, 70_000),
                 small(LINE + MIB + 70_030, SIZE - 64)]
        self.descs = np.concatenate(parts)
        po = self.descs["payload_off"].astype(np.int64)
        pe = po + self.descs["payload_len"].astype(np.int64)
        assert (po[1:] >= pe[:-1]).all() and pe[-1] <= SIZE - 64          # sorted, disjoint, inside the buffer
        assert ((pe <= MIB - 64) | (po >= HI0)).all()                     # inside the two windows
        self.is_lo = pe <= MIB
        self.exp_lo = oracle_regions(self.lo, self.descs[self.is_lo])
        self.exp_hi = oracle_regions(self.hi, self.rel(self.descs[~self.is_lo]))

    @staticmethod
    def rel(descs):
        """Descriptors of the high window, relative to its start."""
        d = descs.copy()
        d["payload_off"] -= HI0
        return d

    def reset(self, hi=None):
        self.buf[:MIB].copy_(torch.from_numpy(self.lo))
        self.buf[HI0:].copy_(torch.from_numpy(self.hi if hi is None else hi))

    def windows(self):
        torch.cuda.synchronize()
        return self.buf[:MIB].cpu().numpy(), self.buf[HI0:].cpu().numpy()

    def middle_is_zero(self):
        """[1 MiB, 2^32 - 1 MiB) on the device, a GiB at a time."""
        return not any(bool(self.buf[s:min(s + (1 << 30), HI0)].any()) for s in range(MIB, HI0, 1 << 30))

    def check_unmasked(self):
        lo, hi = self.windows()
        assert np.array_equal(lo, self.exp_lo)
        assert np.array_equal(hi, self.exp_hi)
        assert self.middle_is_zero()

    def check_untouched(self, hi=None):
        lo, h = self.windows()
        assert np.array_equal(lo, self.lo)
        assert np.array_equal(h, self.hi if hi is None else hi)
        assert self.middle_is_zero()


@pytest.fixture(scope="module")
def far(cuda):
    f = Far(cuda)
    yield f
    f.buf = None
    torch.cuda.empty_cache()


def test_far_regions_cross_the_line(far):
    po = far.descs["payload_off"].astype(np.int64)
    pe = po + far.descs["payload_len"].astype(np.int64)
    assert ((po < LINE) & (pe > LINE)).sum() == 1 and (po >= LINE).sum() > 1000 and far.is_lo.sum() > 1000
    assert far.descs["payload_len"].max() == 100_000 and (far.descs["payload_len"][po >= LINE] == 70_000).any()


@pytest.mark.parametrize("form", ["planned_sorted", "planned_sorted_high", "planned_permuted", "any_sorted",
                                  "any_permuted"])
def test_far_unmask_batch(ctx, cuda, far, hooks, form):
    """fws_gpu_unmask_batch. Both windows in one batch are too sparse for byte space (chunk space,
    k_plan's cbase); the high window's regions alone are planned in byte space with an origin near
    2^32. The any form queues pieces of the two regions over 64 KiB above 2^32."""
    descs, exp_lo = far.descs, far.exp_lo
    if form == "planned_sorted_high":
        descs, exp_lo = descs[~far.is_lo], far.lo
    if form.endswith("permuted"):
        descs = descs[np.random.default_rng(7).permutation(len(descs))]
    hooks.set("unmask_any", form.startswith("any"))
    far.reset()
    gpu.unmask_batch(ctx, far.buf, descs_on(descs, cuda), len(descs))
    lo, hi = far.windows()
    if form.startswith("planned"):
        assert gpu.plan_mode(ctx)["byte_space"] == (1 if form == "planned_sorted_high" else 0)
    assert np.array_equal(lo, exp_lo)
    assert np.array_equal(hi, far.exp_hi)
    assert far.middle_is_zero()


@pytest.mark.parametrize("form", [0, 1, 3], ids=["lookup_first", "early", "xcd_runs"])
def test_far_unmask_sorted(ctx, cuda, far, hooks, form):
    """fws_gpu_unmask_sorted over a span of 4 GiB: 1 Mi units on the grid of the fixture's 1 GiB
    reservation, so every wave takes four turns at the default cap."""
    hooks.set("sorted_early", form)
    far.reset()
    gpu.unmask_sorted(ctx, far.buf, descs_on(far.descs, cuda), len(far.descs))
    far.check_unmasked()


def test_far_unmask_gather(ctx, cuda, far):
    """fws_gpu_unmask_gather with sources in both windows, in any order; the source is not written."""
    rng = np.random.default_rng(11)
    big = np.flatnonzero(far.descs["payload_len"] >= 70_000)
    pick = np.unique(np.concatenate([rng.choice(len(far.descs), 3000, replace=False), big]))
    descs = far.descs[rng.permutation(pick)]
    total = int(descs["payload_len"].sum())
    exp = np.concatenate([(far.exp_lo[o:o + n] if o < MIB else far.exp_hi[o - HI0:o - HI0 + n])
                          for o, n in zip(descs["payload_off"].tolist(), descs["payload_len"].tolist())])
    far.reset()
    dst = torch.zeros(total + 64, dtype=torch.uint8, device=cuda)
    gpu.unmask_gather(ctx, dst, far.buf, descs_on(descs, cuda), len(descs))
    got = dst.cpu().numpy()
    assert np.array_equal(got[:total], exp)
    assert not got[total:].any()
    far.check_untouched()


def test_far_validate_utf8(ctx, cuda, far):
    """fws_gpu_validate_utf8 on the high window's regions holding text, one in five of them with an
    invalid byte. The region across 2^32 is valid and the 70 000-byte one above it is not: an offset
    cut to 32 bits would read random bytes for the first and zeros for the second."""
    rng = np.random.default_rng(13)
    descs = far.descs[~far.is_lo]
    hi = far.hi.copy()
    flags = np.zeros(len(descs), dtype=bool)
    for i, (o, n) in enumerate(zip(descs["payload_off"].tolist(), descs["payload_len"].tolist())):
        body = bytearray(text(rng, n).ljust(n, b"."))
        if n and ((i % 5 == 0 and n != 100_000) or n == 70_000):
            body[int(rng.integers(0, n))] = 0xFF
        hi[o - HI0:o - HI0 + n] = np.frombuffer(bytes(body), dtype=np.uint8)
        flags[i] = valid(body)
    assert flags[descs["payload_len"] == 100_000].all() and not flags[descs["payload_len"] == 70_000].any()
    far.reset(hi)
    ok = torch.full((len(descs),), 7, dtype=torch.uint8, device=cuda)
    gpu.validate_utf8(ctx, far.buf, descs_on(descs, cuda), len(descs), ok)
    okh = ok.cpu().numpy()
    assert set(np.unique(okh)) <= {0, 1}
    assert np.array_equal(okh.astype(bool), flags), np.flatnonzero(okh.astype(bool) != flags)[:10]
    far.check_untouched(hi)


def test_far_mask_4gib_region(cuda, far):
    """fws_gpu_mask on one region of 2^32 + 4096 + 3 bytes at offset 5: the two windows against
    the oracle on the host (the bytes before and after the region included); the zeros between
    them must have become the key at the region's phase, which repeats every four bytes -- the
    word the oracle leaves in a zero buffer at the same offset -- compared on the device."""
    key, off, n = 0xC3A5F00F, 5, LINE + 4096 + 3
    assert HI0 < off + n < SIZE - 64
    far.reset()
    gpu.ws_mask_bytes_fast(far.buf, key, off, n)
    lo, hi = far.windows()
    exp_lo = far.lo.copy()
    orc.orc_mask("ws_mask_fast", exp_lo, key, off, MIB - off)
    assert np.array_equal(lo, exp_lo)
    exp_hi = far.hi.copy()                # the window starts (HI0 - off) bytes into the region
    orc.orc_mask("ws_mask_fast", exp_hi, orc.orc().orc_rotr32(key, 8 * ((HI0 - off) & 3)), 0, off + n - HI0)
    assert np.array_equal(hi, exp_hi)
    z = np.zeros(64, dtype=np.uint8)
    orc.orc_mask("ws_mask_fast", z, key, off, 48)
    word = int(z[8:12].view("<i4")[0])
    assert all(z[p] == z[p + 4] for p in range(off, off + 44))
    for s in range(MIB, HI0, 1 << 30):
        part = far.buf[s:min(s + (1 << 30), HI0)].view(torch.int32)
        assert bool((part == word).all()), hex(s)


def test_zz_far_hooks_are_back_at_their_defaults():
    L = _lib.lib()
    assert L.fws_internal_set_unmask_any(0) == 0
    assert L.fws_internal_set_sorted_early(0) == 0
    assert L.fws_internal_set_grid_cap(0) == 0
