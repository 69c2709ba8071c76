"""Deterministic frame-seam layouts for fws_gpu_encode_frames, and their
classification (pure numpy; no torch, no GPU).

A batch's hard cases are geometric: where a header falls in a 16-B chunk and
in a 4 KiB unit, what its neighbours are, how the source is misaligned against
the output, where the batch ends. `Layout` places frames back to back and
picks a frame's payload length to put the next header at a chosen output
offset; `classify` names, from the descriptors alone, which cells of the class
table (CLASS TABLE below, `required_cells`) a batch contains. The classes are
defined on the layout -- 4 KiB output units counted from output byte 0, 16-B
chunks, a unit "holds two frames" when at most two frames have a byte in it --
not on any kernel's internals, so a rewritten kernel is measured by the same
table. Expected bytes come from the oracle's orc_tx_frame (orc.OrcTx's
builder, pinned to the compiled reference by tests/golden/tx_cases.json.gz).

test_tx_seams_cpu.py asserts that the batches below cover every cell;
test_gpu_tx_seams.py runs them through every form of the kernel.
"""
import ctypes as C
from collections import Counter

import numpy as np

import orc
from flashws_amd._lib import TX_DESC

UNIT, CHUNK = 4096, 16
BIG = UNIT + 1                       # a neighbour "large" enough that no unit holds three such frames
H_ALL = (2, 4, 6, 8, 10, 14)
H_LONG = (4, 8, 10, 14)              # headers of frames over 125 B: such a frame can share a two-frame unit anywhere
C_LIST = (0, 1, 62, 63, 64, 65, 127, 128, 191, 192, 254, 255)
I_LENS = (125, 126, 127, 65535, 65536, 65537)
ONE_TOTALS = (4095, 4096, 4097, 8191, 8192, 8193)
J_COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 16384, 16385)


def hdr_len(n, masked):
    return 2 + (4 if masked else 0) + (0 if n < 126 else 2 if n <= 65535 else 8)


def payload_for(size, masked):
    """The payload length of a frame of `size` bytes in all, or None (no frame
    has that size: e.g. 128 and 129 unmasked)."""
    for ext in (0, 2, 8):
        n = size - 2 - (4 if masked else 0) - ext
        if n >= 0 and hdr_len(n, masked) == size - n:
            return n
    return None


# ------------------------------------------------------------------ the builder
class Batch:
    def __init__(self, name, descs, src, offs, expected):
        self.name, self.descs, self.src, self.offs, self.expected = name, descs, src, offs, expected
        self.total = int(offs[-1])

    def __len__(self):
        return len(self.descs)


class Layout:
    """Frames back to back. add(): one frame; add_to() / next_at(): a frame
    whose payload length puts the next frame's header at a chosen output
    offset. The source holds each payload at a src_off of the residue mod 16
    asked for (`mis`), or at the residue that makes (source address - output
    position of the payload) mod 16 the `shift` asked for; random fill, small
    random gaps, everything from one seeded generator."""

    def __init__(self, seed, name=""):
        self.rng = np.random.default_rng(seed)
        self.name = name
        self.frames = []             # (n, masked, op, fin, key, src_off)
        self.offs = [0]
        self.cur = int(self.rng.integers(0, 16))

    @property
    def pos(self):
        return self.offs[-1]

    def add(self, n, masked=1, op=None, fin=None, key=None, mis=None, shift=None):
        rng = self.rng
        if op is None:
            op = int(rng.choice([1, 2, 0])) if n > 125 else int(rng.choice([0, 1, 2, 8, 9, 10]))
        if fin is None:
            fin = int(rng.random() < 0.5)
        if key is None:
            key = int(rng.integers(0, 1 << 32))
        h = hdr_len(n, masked)
        if shift is not None:
            mis = (self.pos + h + shift) & 15
        so = self.cur + int(rng.integers(0, 40))
        if mis is not None:
            so += (mis - so) & 15
        self.cur = so + n
        self.frames.append((n, int(bool(masked)), op, fin, key, so))
        self.offs.append(self.pos + h + n)
        return len(self.frames) - 1

    def add_to(self, target, masked=1, **kw):
        """A frame ending at output offset `target` (the next header's place)."""
        n = payload_for(target - self.pos, masked)
        if n is None:
            raise ValueError(f"no {'masked' if masked else 'unmasked'} frame of {target - self.pos} bytes")
        return self.add(n, masked, **kw)

    def next_at(self, unit_off, masked=1, min_size=BIG + 3, **kw):
        """A frame of at least min_size bytes ending at the first output offset
        that is `unit_off` bytes into a unit."""
        t = self.pos + min_size
        t += (unit_off - t) % UNIT
        while payload_for(t - self.pos, masked) is None:
            t += UNIT
        return self.add_to(t, masked, **kw)

    def build(self):
        n = len(self.frames)
        d = np.zeros(n, dtype=TX_DESC)
        src = self.rng.integers(0, 256, self.cur + 16, dtype=np.uint8)
        offs = np.array(self.offs, dtype=np.uint64)
        exp = np.zeros(self.pos, dtype=np.uint8)
        fn = orc.orc().orc_tx_frame
        for i, (ln, masked, op, fin, key, so) in enumerate(self.frames):
            d[i] = (so, ln, key, op, fin, masked, 0)
            # orc_tx_frame sequences from its state: a continuation (opcode 0) is a data
            # frame sent while a message is open (tests/test_gpu_tx.py: oracle_frames)
            tx = orc.OrcTx(is_server=not masked)
            tx.state.value = 1 if op == 0 else 0
            k = fn(C.byref(tx.state), tx.is_server, src.ctypes.data + so, ln, 2 if op == 0 else op, fin, key,
                   exp.ctypes.data + self.offs[i])
            assert k == self.offs[i + 1] - self.offs[i], (i, k)
        return Batch(self.name, d, src, offs, exp)


# ------------------------------------------------------------------ CLASS TABLE
# a  ("a", H, r)          a header of H bytes starting r mod 16. H in 4, 8, 10, 14: both neighbours >= 4,097 B
#                         and every unit the header touches holds two frames. H in 2, 6 (a frame <= 125 B):
#                         between two frames >= 4,097 B, which makes a three-frame unit ...
#    ("a_edge", H, r)     ... or as the batch's last frame after a frame >= 4,097 B (a two-frame unit),
#    ("a_first", H)       or as its first frame before one (r is 0 there).
# b  ("b", H, k)          the header has k = 1 .. H - 1 bytes before a 4 KiB boundary (neighbours as in a)
#    ("b_end", H), ("b_start", H)   it ends / starts exactly at the boundary (not the batch's first frame)
# c  ("c", H, c)          H in 4, 8, 10, 14: the header's first chunk is chunk c of its unit (neighbours as in a)
# d  ("d_full" | "d_head" | "d_tail", s, masked)
#                         s = (source address - output position of the payload) mod 16, seen in a two-frame unit
#                         at a full chunk (16 payload bytes of one frame), at the seam chunk holding the
#                         payload's first byte, and at the one holding its last. (Head and tail select
#                         opposite ends of the shifted window, so they are separate cells.)
#    ("d_phase", p)       a masked frame's key phase p at the first payload byte of a full chunk
# e  ("e", 0, k, delta)   two headers 1,024 k + delta apart in one two-frame unit, the first at the unit's
#                         first byte
#    ("e", 16, k, delta)  the first header 16 B into the unit. The bytes before it belong to a third frame,
#                         so this unit cannot hold two frames (units are counted from output byte 0): the cell is
#                         the three-frame unit.
# f  ("f", where, masked, size)   a frame of size = 2 .. 15 B in all (masked: 6 .. 15) at a unit's first byte,
#                         followed by a frame >= 8 KiB; where = "mid" or "first" (the batch's first frame)
# g  ("g", masked, where) an empty frame: "straddle" a unit boundary between two frames >= 4,097 B, "first",
#                         "last" (next to a frame >= 4,097 B), "run20" (>= 20 in a row between two such frames)
# h  ("h_pay", r)         total mod 16 = r, the batch ending in a payload >= 8 KiB
#    ("h_small", r)       ... in a last frame of 0 .. 20 B payload after a frame >= 8 KiB
#    ("h_one", r)         ... in a batch of one frame of 0 .. 40 B payload
#    ("h_total", t)       a one-frame batch of t bytes
# i  ("i", len, masked)   a payload at a length-form edge between two frames >= 4,097 B
# k  ("k", H, r)          H in 4, 8, 10, 14: the header starts r mod 16 and every unit it touches holds three or
#                         more frames (a tiny frame before it: the header is built on the bytewise path)
#    ("k_split", H)       ... it crosses a unit boundary, three or more frames in the left unit, the frame alone
#                         in the right one
#    ("k_tail", H)        ... its payload's last byte lies in a unit of three or more frames (payload bytes at
#                         large frame-relative offsets on the bytewise path). (Classes a-i put long headers in
#                         two-frame units only: a wrong byte of the 64-bit length on the bytewise path passed them.)
# j  frame counts: one batch per n (J_COUNTS), asserted per batch, not a cell
def required_cells():
    cells = [("a", h, r) for h in H_ALL for r in range(16)]
    cells += [("a_edge", h, r) for h in (2, 6) for r in range(16)] + [("a_first", h) for h in (2, 6)]
    cells += [("b", h, k) for h in H_ALL for k in range(1, h)]
    cells += [(t, h) for t in ("b_end", "b_start") for h in H_ALL]
    cells += [("c", h, c) for h in H_LONG for c in C_LIST]
    cells += [(t, s, m) for t in ("d_full", "d_head", "d_tail") for s in range(16) for m in (0, 1)]
    cells += [("d_phase", p) for p in range(4)]
    cells += [("e", v, k, dl) for v in (0, 16) for k in (1, 2, 3) for dl in (0, 1, 15)]
    cells += [("f", w, m, s) for w in ("mid", "first") for m in (0, 1) for s in range(6 if m else 2, 16)]
    cells += [("g", m, w) for m in (0, 1) for w in ("straddle", "first", "last", "run20")]
    cells += [(t, r) for t in ("h_pay", "h_small", "h_one") for r in range(16)]
    cells += [("h_total", t) for t in ONE_TOTALS]
    cells += [("i", ln, m) for ln in I_LENS for m in (0, 1)]
    cells += [("k", h, r) for h in H_LONG for r in range(16)] + [(t, h) for t in ("k_split", "k_tail") for h in H_LONG]
    return cells


def geometry(descs):
    """Per frame: output offset O (n + 1 entries), header length H, payload
    length L, masked M, source offset S; per unit: its first and last frame."""
    L = descs["len"].astype(np.int64)
    M = (descs["masked"] != 0).astype(np.int64)
    H = 2 + 4 * M + np.where(L < 126, 0, np.where(L <= 65535, 2, 8))
    O = np.concatenate([[0], np.cumsum(H + L)]).astype(np.int64)
    total = int(O[-1])
    ustart = np.arange(0, max(total, 1), UNIT, dtype=np.int64)
    uend = np.minimum(ustart + UNIT, total) - 1
    first = np.searchsorted(O, ustart, "right") - 1
    last = np.minimum(np.searchsorted(O, uend, "right") - 1, len(L) - 1)
    return O, H, L, M, descs["src_off"].astype(np.int64), first, last


def classify_events(descs):
    """Every class cell the batch contains, with where: a list of (cell, lo,
    hi), [lo, hi) the output bytes that make the case."""
    n = len(descs)
    ev = []
    if n == 0:
        return ev
    O, H, L, M, S, first, last = geometry(descs)
    total = int(O[-1])
    size = H + L
    two = (last - first) <= 1
    two_cs = np.concatenate([[0], np.cumsum(two)])

    def n_two(lo, hi):                                   # two-frame units among those of bytes [lo, hi)
        return int(two_cs[(hi - 1) // UNIT + 1] - two_cs[lo // UNIT]) if hi > lo else 0

    def all_two(lo, hi):
        return n_two(lo, hi) == (hi - 1) // UNIT - lo // UNIT + 1

    big = size >= BIG
    empty_run = 0
    for i in range(n):
        o, h, ln, m, e = int(O[i]), int(H[i]), int(L[i]), int(M[i]), int(O[i + 1])
        p = o + h
        mid = 0 < i < n - 1 and big[i - 1] and big[i + 1]
        long_h = h in H_LONG
        if mid and (not long_h or all_two(o, p)):
            ev.append((("a", h, o & 15), o, p))
            for k in range(1, h):
                if (o + k) % UNIT == 0:
                    ev.append((("b", h, k), o, p))
            if p % UNIT == 0:
                ev.append((("b_end", h), o, p))
            if o % UNIT == 0:
                ev.append((("b_start", h), o, p))
            if long_h and (o % UNIT) // CHUNK in C_LIST:
                ev.append((("c", h, (o % UNIT) // CHUNK), o, p))
        if long_h and n_two(o, p) == 0:
            ev.append((("k", h, o & 15), o, p))
        if long_h and o // UNIT != (p - 1) // UNIT and last[o // UNIT] - first[o // UNIT] >= 2 and two[p // UNIT]:
            ev.append((("k_split", h), o, p))
        if long_h and last[(e - 1) // UNIT] - first[(e - 1) // UNIT] >= 2:
            ev.append((("k_tail", h), max(p, e - 16), e))
        if not long_h and n >= 2:
            if i == n - 1 and big[i - 1]:
                ev.append((("a_edge", h, o & 15), o, p))
            if i == 0 and big[1]:
                ev.append((("a_first", h), o, p))
        if ln:
            s = (int(S[i]) - p) & 15
            flo, fhi = (p + 15) & ~15, e & ~15
            if n_two(flo, fhi):
                ev.append((("d_full", s, m), flo, fhi))
                if m:
                    ev.append((("d_phase", -p & 3), flo, fhi))
            if p & 15 and two[p // UNIT]:
                ev.append((("d_head", s, m), p, min(e, flo)))
            if e & 15 and fhi >= flo and two[fhi // UNIT]:
                ev.append((("d_tail", s, m), fhi, e))
        if o % UNIT in (0, 16) and i + 1 < n:
            u = o // UNIT
            for k in (1, 2, 3):
                for dl in (0, 1, 15):
                    if size[i] == 1024 * k + dl:
                        if o % UNIT == 0 and two[u]:
                            ev.append((("e", 0, k, dl), o, e + int(H[i + 1])))
                        if o % UNIT == 16 and first[u] == i - 1 and last[u] == i + 1:
                            ev.append((("e", 16, k, dl), o, e + int(H[i + 1])))
        if size[i] <= 15 and o % UNIT == 0 and i + 1 < n and size[i + 1] >= 8192:
            ev.append((("f", "first" if i == 0 else "mid", m, int(size[i])), o, e))
        if ln == 0:
            if o // UNIT != (p - 1) // UNIT and mid:
                ev.append((("g", m, "straddle"), o, p))
            if i == 0 and n >= 2 and big[1]:
                ev.append((("g", m, "first"), o, p))
            if i == n - 1 and n >= 2 and big[i - 1]:
                ev.append((("g", m, "last"), o, p))
            same = empty_run and L[i - 1] == 0 and M[i - 1] == m
            empty_run = empty_run + 1 if same else 1
            run_ends = i + 1 == n or L[i + 1] != 0 or M[i + 1] != m
            r0 = i - empty_run + 1
            if run_ends and empty_run >= 20 and r0 > 0 and big[r0 - 1] and i + 1 < n and big[i + 1]:
                ev.append((("g", m, "run20"), int(O[r0]), p))
        else:
            empty_run = 0
        if ln in I_LENS and mid:
            ev.append((("i", ln, m), o, p))
    tail = ((total - 1) & ~15, total)
    if L[-1] >= 8192:
        ev.append((("h_pay", total & 15),) + tail)
    if n >= 2 and L[-1] <= 20 and size[-2] >= 8192:
        ev.append((("h_small", total & 15),) + tail)
    if n == 1 and L[0] <= 40:
        ev.append((("h_one", total & 15),) + tail)
    if n == 1 and total in ONE_TOTALS:
        ev.append((("h_total", total),) + tail)
    return ev


def classify(descs):
    """Counts per class cell (see CLASS TABLE)."""
    return Counter(c for c, _, _ in classify_events(descs))


def describe_byte(descs, b):
    """Where output byte b lies: frame index, offset in its frame, in its unit,
    in its chunk, the unit's frame count, and the class cells its chunk meets."""
    O, H, L, M, S, first, last = geometry(descs)
    f = int(np.searchsorted(O, b, "right") - 1)
    u = b // UNIT
    c0 = b & ~15
    cells = sorted({str(c) for c, lo, hi in classify_events(descs) if lo < c0 + 16 and hi > c0})
    k = b - int(O[f])
    part = f"header byte {k} of {int(H[f])}" if k < H[f] else f"payload byte {k - int(H[f])} of {int(L[f])}"
    return (f"output byte {b}: frame {f} ({part}, masked={int(M[f])}, src_off%16={int(S[f]) & 15}), "
            f"unit {u} offset {b % UNIT} (chunk {(b % UNIT) // 16}, lane {(b % UNIT) // 16 % 64}, "
            f"holds {int(last[u] - first[u]) + 1} frames), offset {b & 15} in its chunk; "
            f"classes of the chunk: {', '.join(cells) or 'none'}")


# ------------------------------------------------------------------ the batches
def _walk_long(lay, hs):
    """Frames slightly over 4 KiB (H = 4 / 8) or 64 KiB (10 / 14), every frame
    a target: its length puts the next header at the next wanted unit offset."""
    for h in hs:
        masked = h in (8, 14)
        min_size = BIG + 3 if h in (4, 8) else 65536 + 14
        targets = [512 + 16 * r + r for r in range(16)]                    # a: every start mod 16
        targets += [UNIT - k for k in range(1, h)] + [UNIT - h, 0]          # b: every split, ending at, starting at
        targets += [16 * c + (5 * j) % 16 for j, c in enumerate(C_LIST)]    # c: the header's first chunk
        # the frame before the first target, then one frame per target; the frame at a
        # target is of form h, its own length chosen for the next target
        lay.next_at(targets[0], masked=1, min_size=BIG + 3, shift=0)
        for j, t in enumerate(targets):
            assert lay.pos % UNIT == t
            nxt = targets[j + 1] if j + 1 < len(targets) else 100
            lay.next_at(nxt, masked=masked, min_size=min_size, shift=j % 16)
            assert hdr_len(lay.frames[-1][0], masked) == h


def _walk_short(lay):
    """Frames <= 125 B (H = 2 / 6) between frames slightly over 4 KiB."""
    j = 0
    for h in (2, 6):
        masked = h == 6
        targets = [700 + 16 * r + r for r in range(16)]
        targets += [UNIT - k for k in range(1, h)] + [UNIT - h, 0]
        for t in targets:
            lay.next_at(t, masked=j & 1, shift=(3 * j) % 16)
            lay.add([0, 1, 7, 16, 33, 125][j % 6], masked=masked, shift=(5 * j) % 16)
            j += 1
    lay.next_at(33, masked=1, shift=9)


def batch_abcd():
    """Classes a-d: headers of every length at every start mod 16, across and
    at unit boundaries, at the chunk indices of C_LIST; every shift and phase."""
    lay = Layout(101, "abcd")
    lay.add(5000, masked=0, shift=3)
    _walk_long(lay, (4, 8))
    _walk_short(lay)
    _walk_long(lay, (10, 14))
    lay.add(4500, masked=1, shift=11)
    return lay.build()


def batch_efi():
    """Classes e, f (mid) and i."""
    lay = Layout(102, "efi")
    lay.add(6000, masked=1, shift=5)
    j = 0
    for k in (1, 2, 3):                                   # e: A at the unit's first byte, B 1,024 k + delta after
        for dl in (0, 1, 15):
            lay.next_at(0, masked=j & 1, shift=j % 16)
            lay.add_to(lay.pos + 1024 * k + dl, masked=(j >> 1) & 1, shift=(7 * j) % 16)
            lay.next_at(100 + j, masked=(j + 1) & 1, shift=(3 * j) % 16)
            j += 1
    for k in (1, 2, 3):                                   # e, 16 B into the unit: after 16 B of a third frame
        for dl in (0, 1, 15):
            lay.next_at(16, masked=j & 1, shift=j % 16)
            lay.add_to(lay.pos + 1024 * k + dl, masked=(j >> 1) & 1, shift=(7 * j) % 16)
            lay.next_at(200 + j, masked=(j + 1) & 1, shift=(3 * j) % 16)
            j += 1
    for masked in (0, 1):                                 # f: a tiny frame at a unit's first byte, then >= 8 KiB
        for size in range(6 if masked else 2, 16):
            lay.next_at(0, masked=j & 1, shift=j % 16)
            lay.add(payload_for(size, masked), masked=masked, shift=(5 * j) % 16)
            lay.add(8192 + 37 * j, masked=(j >> 1) & 1, shift=(11 * j) % 16)
            j += 1
    for ln in I_LENS:                                     # i: length-form edges between large frames
        for masked in (0, 1):
            lay.add(4200 + 13 * j, masked=j & 1, shift=j % 16)
            lay.add(ln, masked=masked, shift=(9 * j) % 16)
            j += 1
    lay.add(4321, masked=0, shift=14)
    return lay.build()


def batch_k():
    """Class k: long headers after a tiny frame, in units of three frames."""
    lay = Layout(106, "k")
    lay.add(5000, masked=1, shift=6)
    j = 0
    for h in H_LONG:
        masked = h in (8, 14)
        for r in list(range(16)) + ["split"]:
            tiny = 2 + j % 11                              # an unmasked frame of 2 .. 12 B
            uo = UNIT - tiny - 1 - j % (h - 1) if r == "split" else 160 * (1 + j % 20) + (r - tiny) % 16
            lay.next_at(uo, masked=j & 1, shift=j % 16)
            lay.add(tiny - 2, masked=0, shift=(3 * j) % 16)
            lay.add((4200 if h in (4, 8) else 65536) + 7 * j, masked=masked, shift=(5 * j) % 16)
            if r in (3, 12):                               # the long frame's tail in a three-frame unit too
                lay.add(j % 9, masked=j & 1, shift=(7 * j) % 16)
            j += 1
    lay.add(4300, masked=0, shift=1)
    return lay.build()


def batch_g(flip):
    """Class g: empty frames straddling a unit boundary, in runs of 20, as the
    batch's first and last frame (flip = 0: first masked, last unmasked; 1: the
    other way round, the small second batch)."""
    lay = Layout(103 + flip, f"g{flip}")
    lay.add(0, masked=1 - flip)
    lay.add(5000, masked=flip, shift=2)
    if not flip:
        for j, (masked, back) in enumerate([(0, 1), (1, 1), (1, 2), (1, 3), (1, 4), (1, 5)]):
            lay.next_at(UNIT - back, masked=j & 1, shift=(3 * j + 1) % 16)      # the header starts `back` B before
            lay.add(0, masked=masked)
            lay.add(4100 + 7 * j, masked=(j + 1) & 1, shift=(5 * j) % 16)
        for masked in (0, 1):
            for _ in range(20):
                lay.add(0, masked=masked)
            lay.add(4200, masked=masked, shift=7 + masked)
        for _ in range(23):                                                     # a mixed run, not a cell
            lay.add(0, masked=int(lay.rng.integers(0, 2)))
        lay.add(9000, masked=0, shift=13)
    lay.add(0, masked=flip)
    return lay.build()


def batch_spans():
    """For the one-launch form at 8 frames per workgroup: groups of 8 frames
    whose span ends r = 1 .. 15 past a chunk boundary, each followed by 16
    unmasked empty frames (two more spans, each 16 B, so every span ends off
    chunk alignment and the next starts with 2-byte frames: the look-ahead of
    8 frames is exactly what a chunk's 15 bytes past the span can meet)."""
    lay = Layout(105, "spans")
    for kind in (0, 1):
        for r in range(1, 16):
            sizes = ([5000 + 31 * r, 3, 130, 0, 17, 4096, 1, 60] if kind else [40 + r, 0, 125, 126, 9, 300, 2, 31])
            for j, ln in enumerate(sizes[:7]):
                lay.add(ln, masked=(j + r + kind) & 1, shift=(j + r) % 16)
            want = (r - lay.pos) & 15                     # the last frame's size: the span ends at r mod 16
            masked = r & 1
            size = 64 + want
            lay.add(payload_for(size, masked), masked=masked, shift=(3 * r) % 16)
            assert lay.pos & 15 == r
            for _ in range(16):
                lay.add(0, masked=0)
    lay.add(777, masked=1, shift=4)
    return lay.build()


def batch_count(n):
    """Class j: n frames of 0 .. 40 B."""
    lay = Layout(200 + n, f"n{n}")
    for _ in range(n):
        lay.add(int(lay.rng.integers(0, 41)), masked=int(lay.rng.random() < 0.7))
    return lay.build()


def end_batches():
    """Class h, the a_edge / a_first cells and f "first": many tiny batches."""
    out = []
    for r in range(16):                                   # the end inside a payload >= 8 KiB
        lay = Layout(300 + r, f"h_pay{r}")
        lay.add(4100 + r, masked=r & 1, shift=r)
        masked = (r >> 1) & 1
        lay.add_to(lay.pos + 8192 + 14 + 16 + ((r - lay.pos - 14) & 15), masked=masked, shift=(5 * r) % 16)
        assert lay.pos & 15 == r and lay.frames[-1][0] >= 8192
        out.append(lay.build())
    for r in range(16):                                   # a last frame of 0 .. 20 B at every start mod 16
        for ln in range(21):
            masked = (r + ln) & 1
            lay = Layout(400 + 32 * r + ln, f"h_small{r}_{ln}")
            lay.add_to(8192 + 16 + r, masked=(ln >> 1) & 1, shift=(r + ln) % 16)
            lay.add(ln, masked=masked, shift=(3 * ln + r) % 16)
            out.append(lay.build())
    for ln in range(41):                                  # one frame of 0 .. 40 B
        for masked in (0, 1):
            lay = Layout(1000 + 2 * ln + masked, f"h_one{ln}_{masked}")
            lay.add(ln, masked=masked, shift=(ln + masked) % 16)
            out.append(lay.build())
    for t in ONE_TOTALS:                                  # one frame of t bytes
        for masked in (0, 1):
            lay = Layout(1100 + t + masked, f"h_total{t}_{masked}")
            lay.add_to(t, masked=masked, shift=(t + 5 * masked) % 16)
            out.append(lay.build())
    for masked in (0, 1):                                 # a tiny first frame, then >= 8 KiB
        for size in range(6 if masked else 2, 16):
            lay = Layout(1200 + 16 * masked + size, f"f_first{size}_{masked}")
            lay.add(payload_for(size, masked), masked=masked, shift=size)
            lay.add(8192 + size, masked=size & 1, shift=(7 * size) % 16)
            out.append(lay.build())
    return out


SEAM_BATCHES = {"abcd": batch_abcd, "efi": batch_efi, "g0": lambda: batch_g(0), "g1": lambda: batch_g(1),
                "k": batch_k, "spans": batch_spans}

_cache = {}


def get_batch(name):
    """The batch of that name, built once and shared (never modified)."""
    if name not in _cache:
        if name == "ends":
            _cache[name] = end_batches()
        elif name in SEAM_BATCHES:
            _cache[name] = SEAM_BATCHES[name]()
        else:
            _cache[name] = batch_count(int(name[1:]))
        for b in (_cache[name] if isinstance(_cache[name], list) else [_cache[name]]):
            for a in (b.descs, b.src, b.offs, b.expected):
                a.setflags(write=False)
    return _cache[name]


def all_batches():
    """Every batch the GPU tests run."""
    out = [get_batch(k) for k in SEAM_BATCHES] + [get_batch(f"n{n}") for n in J_COUNTS]
    return out + get_batch("ends")
