"""Deterministic region-seam layouts for fws_gpu_unmask_gather, and their
classification (pure numpy; no torch, no GPU).

The gather's hard cases are geometric: where two regions meet inside a 16-B
output chunk and inside a 4 KiB unit, how each side's source is misaligned
against the output, the key phase on each side, where the output ends, where
the sources lie in `src`. `Layout` places regions in destination order, picks a
region's length to put the next seam (the destination prefix B) at a chosen
offset, and gives each source either a chosen payload_off mod 16 or a chosen
shift, (source address - B_i) mod 16. `classify` names, from the descriptors
alone (plus len(src) and the view's skew for class g), which cells of the class
table (CLASS TABLE below, `required_cells`) a batch contains. The classes are
defined on the layout -- 4 KiB output units counted from dst byte 0, 16-B
chunks, a unit "holds two regions" when at most two non-empty regions have a
byte in it -- not on any kernel's internals, so a rewritten kernel is measured
by the same table.

Expected bytes are a vectorised restatement of the operation,
dst[B_i + k] = src[payload_off_i + k] ^ byte((k + phase_i) & 3) of key_i;
test_gather_seams_cpu.py pins it to the oracle's ws_mask_fast per region and
asserts that the batches below cover every cell; test_gpu_gather_seams.py runs
them through every form of the kernel.
"""
from collections import Counter

import numpy as np

from flashws_amd._lib import FRAME_DESC

UNIT, CHUNK = 4096, 16
BIG = UNIT + 1                       # "big": no unit holds three such regions
C_LIST = (0, 1, 62, 63, 64, 65, 127, 128, 191, 192, 254, 255)
C_POS = (0, 1, 8, 15)
C_UNIT = (0, 1, 15, -1, -15)         # the seam's distance from a unit boundary
D_TOTALS = (1, 15, 16, 17, 4095, 4096, 4097, 8192)
F_RUNS = range(34)
G_SKEWS = (1, 7, 15)
H_COUNTS = (1, 2, 3, 2047, 2048, 2049)


def _pairs16():
    """A cyclic sequence of 256 values 0..15 in which every ordered pair occurs
    once as neighbours (the Lyndon words of length 1 and 2 in order)."""
    seq = []
    for i in range(16):
        seq.append(i)
        for j in range(i + 1, 16):
            seq += [i, j]
    return seq


# ------------------------------------------------------------------ the builder
class Batch:
    def __init__(self, name, descs, src, B, expected, skew=0):
        self.name, self.descs, self.src, self.B, self.expected, self.skew = name, descs, src, B, expected, skew
        self.total = int(B[-1])

    def __len__(self):
        return len(self.descs)


def expected_of(descs, src):
    """dst[B_i + k] = src[payload_off_i + k] ^ byte((k + phase_i) & 3) of key_i."""
    n = len(descs)
    L = descs["payload_len"].astype(np.int64)
    B = np.concatenate([[0], np.cumsum(L)])
    idx = np.repeat(np.arange(n), L)
    k = np.arange(int(B[-1]), dtype=np.int64) - B[idx]
    s = src[descs["payload_off"].astype(np.int64)[idx] + k]
    sh = (((k + descs["phase"].astype(np.int64)[idx]) & 3) * 8).astype(np.uint32)
    return s ^ ((descs["key"].astype(np.uint32)[idx] >> sh) & 0xFF).astype(np.uint8)


class Layout:
    """Regions in destination order. add(): one region; add_to() / next_at() /
    next_mod16(): a region whose length puts the next seam at a chosen place.
    A region's source starts at the payload_off residue mod 16 asked for
    (`mis`), or at the one that makes (source address - B_i) mod 16 the `shift`
    asked for (the address counts the view's `skew` into its 16-B-aligned
    tensor); `gap` bytes after the source before it (None: 0 .. 39 at random,
    0 with no mis / shift: adjacent). order "perm" lays the sources out in a
    random order; lead / tail: the bytes of src before the first and after the
    last source (None: a few at random; 0: a source at src's first / last
    byte). Everything from one seeded generator."""

    def __init__(self, seed, name="", skew=0, lead=None, tail=None, order="dst"):
        self.rng = np.random.default_rng(seed)
        self.name, self.skew, self.lead, self.tail, self.order = name, skew, lead, tail, order
        self.regs = []               # (len, key, phase, mis, gap)
        self.B = [0]

    @property
    def pos(self):
        return self.B[-1]

    def add(self, n, key=None, phase=None, mis=None, shift=None, gap=None):
        rng = self.rng
        if key is None:
            key = int(rng.integers(0, 1 << 32))
        if phase is None:
            phase = int(rng.integers(0, 4))
        if shift is not None:
            mis = (self.pos + shift - self.skew) & 15
        self.regs.append((int(n), key, phase, mis, gap))
        self.B.append(self.pos + int(n))
        return len(self.regs) - 1

    def add_to(self, target, **kw):
        """A region ending at destination offset `target` (the next seam)."""
        assert target >= self.pos
        return self.add(target - self.pos, **kw)

    def next_at(self, unit_off, min_len=BIG, **kw):
        """A region of at least min_len bytes ending at the first destination
        offset that is `unit_off` bytes into a unit."""
        t = self.pos + min_len
        return self.add_to(t + (unit_off - t) % UNIT, **kw)

    def next_mod16(self, p, min_len=BIG, **kw):
        """... ending at the first offset that is p mod 16."""
        t = self.pos + min_len
        return self.add_to(t + (p - t) % 16, **kw)

    def build(self):
        rng, n = self.rng, len(self.regs)
        order = rng.permutation(n) if self.order == "perm" else np.arange(n)
        cur = int(rng.integers(0, 16)) if self.lead is None else self.lead
        offs = np.zeros(n, dtype=np.int64)
        for j, i in enumerate(order):
            ln, _, _, mis, gap = self.regs[i]
            # (an empty region takes no gap of its own; the first source follows a chosen lead directly)
            so = cur + (int(rng.integers(0, 40)) if gap is None and ln and (j or self.lead is None) else (gap or 0))
            if mis is not None:
                so += (mis - so) & 15
            offs[i] = so
            cur = so + ln
        src = rng.integers(0, 256, cur + (int(rng.integers(16, 48)) if self.tail is None else self.tail),
                           dtype=np.uint8)
        d = np.zeros(n, dtype=FRAME_DESC)
        for i, (ln, key, phase, _, _) in enumerate(self.regs):
            d[i] = (offs[i], ln, key, phase)
        return Batch(self.name, d, src, np.array(self.B, dtype=np.uint64), expected_of(d, src), self.skew)


# ------------------------------------------------------------------ CLASS TABLE
# Shifts and source residues are taken from the real address, skew + payload_off.
# a  ("a", p, sl, sr)     a seam B between two big regions (both >= 4,097 B, neighbours in the descriptors: the
#                         units it touches hold two regions), p = B mod 16, sl / sr the left / right region's shift.
#                         p = 0 is the seam on a chunk boundary.
# b  ("b", B mod 4, (len_left + phase_left) mod 4, phase_right)   the key phases at such a seam
# c  ("c", c, p, nz)      such a seam whose chunk (the one holding byte B) is chunk c of its unit, p in 0, 1, 8, 15,
#                         nz = the left shift is non-zero
#    ("c_unit", k)        B mod 4096 = k mod 4096, k in 0, +-1, +-15
# d  ("d_in", r)          total mod 16 = r, the last chunk inside one big region
#    ("d_seam", r)        ... the last region 1 .. 15 B after a big one, the seam in the last chunk
#    ("d_zero", r, z)     ... z = 1 or 2 zero-length regions after a big last one
#    ("d_total", t)       the batch's total
# e  ("e_first", m, x)    a region of 1 .. 15 B as the batch's first, before a big one, in a unit that holds two
#                         regions: source residue m mod 16, x = it straddles two 16-B source blocks (m + len > 16)
#    ("e_last", m, x)     ... as the batch's last, after a big one
# f  ("f_run", len, m)    a region of len = 0 .. 33 B at source residue m, every unit it touches holding three or
#                         more regions
#    ("f_ones",)          an aligned chunk of 16 one-byte regions
#    ("f_zeros",)         a chunk with bytes of three regions, zero-length ones between them
#    ("f_before",), ("f_after",)   a unit of three or more regions directly before / after a unit that holds one
#    ("f_full", s)        a chunk of 16 B of one region at shift s in a unit of three or more regions
#    ("f_phase", q)       ... the key phase q at its first byte
# g  ("g_src0",), ("g_end",)   a source at src's first byte / ending at its last
#    ("g_adjacent",)      two sources with no byte between them
#    ("g_perm",)          sources not in destination order
#    ("g_skew", k)        src a view k = 1, 7, 15 B into its 16-B-aligned tensor
# h  ("h", n)             the region count
def required_cells():
    cells = [("a", p, sl, sr) for p in range(16) for sl in range(16) for sr in range(16)]
    cells += [("b", x, y, z) for x in range(4) for y in range(4) for z in range(4)]
    cells += [("c", c, p, nz) for c in C_LIST for p in C_POS for nz in (0, 1)] + [("c_unit", k) for k in C_UNIT]
    cells += [(t, r) for t in ("d_in", "d_seam") for r in range(16)]
    cells += [("d_zero", r, z) for r in range(16) for z in (1, 2)] + [("d_total", t) for t in D_TOTALS]
    cells += [(t, m, x) for t in ("e_first", "e_last") for m in range(16) for x in (0, 1) if not x or m >= 2]
    cells += [("f_run", ln, m) for ln in F_RUNS for m in range(16)]
    cells += [("f_ones",), ("f_zeros",), ("f_before",), ("f_after",)]
    cells += [("f_full", s) for s in range(16)] + [("f_phase", q) for q in range(4)]
    cells += [("g_src0",), ("g_end",), ("g_adjacent",), ("g_perm",)] + [("g_skew", k) for k in G_SKEWS]
    cells += [("h", n) for n in H_COUNTS]
    return cells


def geometry(descs, skew=0):
    """Per region: length L, prefix B (n + 1), source offset S, phase P, shift,
    source residue; per unit: how many non-empty regions have a byte in it."""
    L = descs["payload_len"].astype(np.int64)
    B = np.concatenate([[0], np.cumsum(L)]).astype(np.int64)
    S = descs["payload_off"].astype(np.int64)
    total = int(B[-1])
    ne = np.flatnonzero(L > 0)
    ustart = np.arange(0, max(total, 1), UNIT, dtype=np.int64)
    uend = np.maximum(np.minimum(ustart + UNIT, total) - 1, 0)
    cnt = np.searchsorted(B[ne], uend, "right") - np.searchsorted(B[ne], ustart, "right") + 1 if total else ustart * 0
    return L, B, S, descs["phase"].astype(np.int64), (skew + S - B[:-1]) & 15, (skew + S) & 15, cnt


def classify_events(descs, src_len=None, skew=0):
    """Every class cell the batch contains, with where: a list of (cell, lo,
    hi), [lo, hi) the destination bytes that make the case."""
    n = len(descs)
    ev = []
    if n == 0:
        return ev
    L, B, S, P, shift, mis, cnt = geometry(descs, skew)
    total = int(B[-1])
    big = L >= BIG
    for i in np.flatnonzero(big[:-1] & big[1:]):
        b = int(B[i + 1])
        p, lo = b & 15, (b - 1) & ~15
        span = (lo, (b & ~15) + 16)
        ev.append((("a", p, int(shift[i]), int(shift[i + 1])),) + span)
        ev.append((("b", b & 3, int(L[i] + P[i]) & 3, int(P[i + 1]) & 3),) + span)
        c = (b % UNIT) // CHUNK
        if c in C_LIST and p in C_POS:
            ev.append((("c", c, p, int(shift[i] != 0)),) + span)
        for k in C_UNIT:
            if b % UNIT == k % UNIT:
                ev.append((("c_unit", k),) + span)
    if total:
        r, tail = total & 15, ((total - 1) & ~15, total)
        z = 0
        while L[n - 1 - z] == 0:
            z += 1
        if z == 0 and big[-1]:
            ev.append((("d_in", r),) + tail)
        if z == 0 and n >= 2 and 1 <= L[-1] <= 15 and big[-2] and B[-2] >= tail[0]:
            ev.append((("d_seam", r),) + tail)
        if z in (1, 2) and big[n - 1 - z]:
            ev.append((("d_zero", r, z),) + tail)
        if total in D_TOTALS:
            ev.append((("d_total", total),) + tail)
        if n >= 2 and 1 <= L[0] <= 15 and big[1] and cnt[0] <= 2:
            ev.append((("e_first", int(mis[0]), int(mis[0] + L[0] > 16)), 0, int(L[0])))
        if n >= 2 and 1 <= L[-1] <= 15 and big[-2] and cnt[-1] <= 2:
            ev.append((("e_last", int(mis[-1]), int(mis[-1] + L[-1] > 16)), int(B[-2]), total))
        many = cnt >= 3
        if many.any():
            for i in np.flatnonzero(L <= 33):
                b, e = int(B[i]), int(B[i + 1])
                u0, u1 = min(b, total - 1) // UNIT, (max(e, b + 1) - 1) // UNIT if e > b else min(b, total - 1) // UNIT
                if many[u0:u1 + 1].all():
                    ev.append((("f_run", int(L[i]), int(mis[i])), b, max(e, b + 1)))
            for i in np.flatnonzero((L > 16) & (L < UNIT)):
                flo, fhi = (int(B[i]) + 15) & ~15, int(B[i + 1]) & ~15
                if fhi > flo and many[flo // UNIT]:
                    ev.append((("f_full", int(shift[i])), flo, flo + 16))
                    ev.append((("f_phase", int(flo - B[i] + P[i]) & 3), flo, flo + 16))
            one = (L == 1).astype(np.int64)
            run16 = np.convolve(one, np.ones(16, dtype=np.int64), "valid") == 16 if n >= 16 else np.zeros(0, bool)
            for i in np.flatnonzero(run16):
                if B[i] % 16 == 0 and many[int(B[i]) // UNIT]:
                    ev.append((("f_ones",), int(B[i]), int(B[i]) + 16))
            for j in range(1, n - 1):
                a = int(B[j]) & ~15
                if L[j] and not L[j - 1] and not L[j + 1] and a < B[j] and B[j + 1] < min(a + 16, total):
                    ev.append((("f_zeros",), a, a + 16))
            for u in np.flatnonzero(many):
                if u + 1 < len(cnt) and cnt[u + 1] == 1:
                    ev.append((("f_before",), int(u) * UNIT, int(u + 1) * UNIT))
                if u >= 1 and cnt[u - 1] == 1:
                    ev.append((("f_after",), int(u) * UNIT, min(int(u + 1) * UNIT, total)))
    if src_len is not None:
        ne = np.flatnonzero(L > 0)
        so, sl = S[ne], L[ne]
        if (so == 0).any():
            ev.append((("g_src0",), 0, 0))
        if (so + sl == src_len).any():
            ev.append((("g_end",), 0, 0))
        o = np.argsort(so)
        if (so[o][1:] == (so + sl)[o][:-1]).any():
            ev.append((("g_adjacent",), 0, 0))
        if (np.diff(so) < 0).any():
            ev.append((("g_perm",), 0, 0))
    if skew in G_SKEWS:
        ev.append((("g_skew", skew), 0, 0))
    if n in H_COUNTS:
        ev.append((("h", n), 0, 0))
    return ev


def classify(descs, src_len=None, skew=0):
    """Counts per class cell (see CLASS TABLE)."""
    return Counter(c for c, _, _ in classify_events(descs, src_len, skew))


def describe_byte(descs, x, skew=0):
    """Where destination byte x lies: region index, offset in its region, in
    its unit and chunk, the unit's region count, and the class cells its chunk
    meets."""
    L, B, S, P, shift, mis, cnt = geometry(descs, skew)
    ne = np.flatnonzero(L > 0)
    f = int(ne[np.searchsorted(B[ne], x, "right") - 1])
    u, c0 = x // UNIT, x & ~15
    cells = sorted({str(c) for c, lo, hi in classify_events(descs, None, skew) if lo < c0 + 16 and hi > c0})
    return (f"dst byte {x}: region {f} (byte {x - int(B[f])} of {int(L[f])}, shift {int(shift[f])}, "
            f"source residue {int(mis[f])}, phase {int(P[f])}), unit {u} offset {x % UNIT} (chunk {(x % UNIT) // 16}, "
            f"lane {(x % UNIT) // 16 % 64}, holds {int(cnt[u])} regions), offset {x & 15} in its chunk; "
            f"classes of the chunk: {', '.join(cells) or 'none'}")


# ------------------------------------------------------------------ the batches
def batch_a(q):
    """Class a, seam positions 4 q .. 4 q + 3: a chain of big regions, every
    region the right side of one seam and the left side of the next; per
    position the shifts walk a cycle through all 256 (left, right) pairs."""
    lay = Layout(500 + q, f"a{q}", order="perm" if q & 1 else "dst")
    seq = _pairs16()
    first = True
    for p in range(4 * q, 4 * q + 4):
        for t in range(257 if first else 256):
            # the region with this shift ends at the next seam of position p; a few chunks more at random move
            # the seams through the unit
            s = seq[(t if first else t + 1) % 256]
            if first and t == 0:
                lay.add(int(lay.rng.integers(0, 16)))          # a short head: the chain's first seam mod 16 = p
                lay.next_mod16(p, shift=s)
                continue
            last_of_p = t == (256 if first else 255)
            nxt = p + 1 if last_of_p and p < 4 * q + 3 else p
            lay.next_mod16(nxt, min_len=BIG + 16 * int(lay.rng.integers(0, 24)), shift=s)
        first = False
    if q == 3:
        # class c once more behind 4 MiB of output, where a grid of one workgroup is past every wave's 64th unit
        _walk_c(lay)
        lay.add(4400, shift=7)
    return lay.build()


def _walk_c(lay):
    """Seams of big regions in the chunks of C_LIST at positions 0, 1, 8, 15
    with a zero and a non-zero left shift, and at and next to a unit boundary."""
    j = 0
    for c in C_LIST:
        for p in C_POS:
            for nz in (0, 1):
                # the region ending at the wanted seam is its left side
                lay.next_at(16 * c + p, shift=(1 + j % 15) if nz else 0)
                j += 1
    for k in C_UNIT:
        lay.next_at(k % UNIT, shift=(5 * j) % 16)
        j += 1
    return j


def batch_bc():
    """Classes b and c: every key-phase combination at a seam of two big
    regions; seams in the chunks of C_LIST at positions 0, 1, 8, 15 with a zero
    and a non-zero left shift; seams at and next to a unit boundary."""
    lay = Layout(510, "bc")
    lay.add(5000, shift=3)
    j = _walk_c(lay)
    for x in range(4):
        for y in range(4):
            for z in range(4):
                ln = BIG + 16 * (j % 9)
                ln += (x - (lay.pos + ln)) & 3                    # the seam's B mod 4 = x
                lay.add(ln, phase=(y - ln) & 3, shift=(3 * j) % 16)
                lay.add(BIG + 7 * j % 64, phase=z, shift=(7 * j) % 16)
                j += 1
    lay.add(4500, shift=11)
    return lay.build()


def end_batches():
    """Class d: every total mod 16 with the end inside a big region, in a
    last region of 1 .. 15 B, before one and two zero-length regions; the
    totals of D_TOTALS as one region and as three."""
    out = []
    for r in range(16):
        lay = Layout(600 + r, f"d_in{r}")
        lay.add(4100 + 3 * r, shift=r)
        lay.next_mod16(r, shift=(5 * r) % 16)
        out.append(lay.build())
        lay = Layout(620 + r, f"d_seam{r}")
        tiny = 1 + (r + 14) % 15 if r == 0 else 1 + (7 * r) % r      # r = 0: 1 .. 15; else 1 .. r, inside the last chunk
        lay.next_mod16((r - tiny) & 15, shift=(3 * r) % 16)
        lay.add(tiny, shift=(11 * r) % 16)
        out.append(lay.build())
        for z in (1, 2):
            lay = Layout(640 + 2 * r + z, f"d_zero{r}_{z}")
            if r & 1:
                lay.add(300 + r, shift=r)
            lay.next_mod16(r, shift=(7 * r + z) % 16)
            for _ in range(z):
                lay.add(0)
            out.append(lay.build())
    for t in D_TOTALS:
        lay = Layout(700 + t, f"d_total{t}")
        lay.add(t, shift=t % 16)
        out.append(lay.build())
        if t >= 3:
            lay = Layout(720 + t, f"d_total{t}_3")
            lay.add(t // 3, shift=(t + 1) % 16)
            lay.add(t // 2 - t // 3, shift=(t + 6) % 16)
            lay.add_to(t, shift=(t + 11) % 16)
            out.append(lay.build())
    return out


def tiny_batches():
    """Class e: a region of 1 .. 15 B as the first / last region beside a big
    one, at every source residue, inside one source block and across two."""
    out = []
    for m in range(16):
        for x in (0, 1):
            if x and m < 2:
                continue
            ln = (17 - m + (m * 5) % (m - 1)) if x else 1 + (3 * m) % (16 - m)     # x: m + ln > 16, ln <= 15
            assert 1 <= ln <= 15 and (m + ln > 16) == bool(x)
            lay = Layout(800 + 2 * m + x, f"e_first{m}_{x}")
            lay.add(ln, mis=m)
            lay.add(4200 + 5 * m, shift=(7 * m + x) % 16)
            out.append(lay.build())
            lay = Layout(840 + 2 * m + x, f"e_last{m}_{x}")
            lay.add(4300 + 9 * m + x, shift=(3 * m + x) % 16)
            lay.add(ln, mis=m)
            out.append(lay.build())
    return out


def batch_f():
    """Class f: units of three or more regions. Runs of 0 .. 33 B at every
    source residue; mid-sized regions (full chunks on the search path) at every
    shift and phase; a chunk of 16 one-byte regions; a chunk of three regions
    with zero-length ones between them; such units directly before and after
    units that hold one region."""
    lay = Layout(520, "f")
    lay.add(4200, shift=5)
    for m in range(16):
        for ln in F_RUNS:
            lay.add(ln, mis=m)
    for j in range(48):
        lay.add(900 + 37 * j % 700, shift=j % 16, phase=j % 4)
    lay.add((-lay.pos) % 16 + 16, shift=2)                     # to a chunk boundary
    for _ in range(16):
        lay.add(1)
    for ln in (5, 0, 0, 4, 0, 6, 1):                           # one chunk: 5 | 4 | 6 | 1 with empty regions between
        lay.add(ln)
    for rep in range(2):
        # small regions up to a unit boundary, two units of one region, small regions from the boundary on
        lay.next_at(UNIT - 120, min_len=200, shift=9 + rep)
        for j in range(12):
            lay.add(10, shift=(j + rep) % 16)
        assert lay.pos % UNIT == 0
        lay.add(2 * UNIT, shift=13 - rep)
        for j in range(12):
            lay.add(1 + 3 * j, shift=(5 * j + rep) % 16)
    lay.add(700, shift=4)
    return lay.build()


def place_batches():
    """Class g: sources at src's first and last byte, adjacent, permuted; the
    same kind of layout with src a view 1, 7 and 15 B into its tensor."""
    out = []
    for skew in (0,) + G_SKEWS:
        for order in ("dst", "perm"):
            lay = Layout(900 + 2 * skew + (order == "perm"), f"g_{order}{skew}", skew=skew, lead=0, tail=0,
                         order=order)
            j = 0
            for p in (0, 1, 8, 15, 5):
                for sl in (0, 3, 9, 15):
                    lay.next_mod16(p, shift=sl)
                    j += 1
            lay.add(7, gap=0)
            for ln in (4097, 33, 0, 1, 4200, 16):               # sources with no byte between them
                lay.add(ln, gap=0)
            lay.next_mod16(11, shift=6)
            lay.add(9, gap=0)
            out.append(lay.build())
        # a one-byte region at src's only byte; a tiny region at each end of src around a big one
        lay = Layout(950 + skew, f"g_one{skew}", skew=skew, lead=0, tail=0)
        lay.add(1)
        out.append(lay.build())
        lay = Layout(960 + skew, f"g_ends{skew}", skew=skew, lead=0, tail=0)
        lay.add(3, gap=0)
        lay.add(4111, gap=0)
        lay.add(2, gap=0)
        out.append(lay.build())
    return out


def batch_count(n):
    """Class h: n regions, mostly small, some across several units."""
    lay = Layout(1000 + n, f"n{n}")
    lens = lay.rng.choice([0, 1, 5, 15, 16, 17, 33, 100, 700, 4097], n)
    for ln in lens:
        lay.add(int(ln))
    return lay.build()


FAMILIES = {
    "a": lambda: [batch_a(q) for q in range(4)],
    "bc": lambda: [batch_bc()],
    "d": end_batches,
    "e": tiny_batches,
    "f": lambda: [batch_f()],
    "g": place_batches,
    "h": lambda: [batch_count(n) for n in H_COUNTS],
}

_cache = {}


def get_batch(name):
    """The batches of the family of that name, built once and shared (never
    modified)."""
    if name not in _cache:
        _cache[name] = FAMILIES[name]()
        for b in _cache[name]:
            for a in (b.descs, b.src, b.B, b.expected):
                a.setflags(write=False)
    return _cache[name]


def all_batches():
    """Every batch the GPU tests run."""
    return [b for k in FAMILIES for b in get_batch(k)]
