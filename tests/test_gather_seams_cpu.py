"""The gather seam sweep's own guard (no GPU): the batches
test_gpu_gather_seams.py runs contain every cell of the class table of
gather_seams.py, the builder puts seams, shifts and sources where asked, and
the numpy restatement of the expected bytes equals the oracle's ws_mask_fast
with the key rotated to each region's phase.

The coverage test is what keeps the sweep from covering less as someone edits
it: no sampling, no allowance for a missing cell.
"""
from collections import Counter

import numpy as np

import gather_seams as gs
import orc


def test_every_class_cell_is_covered():
    got = Counter()
    for b in gs.all_batches():
        got.update(gs.classify(b.descs, len(b.src), b.skew))
    missing = [c for c in gs.required_cells() if got[c] < 1]
    assert not missing, f"{len(missing)} cells without a batch: {missing}"


def test_required_cells_table():
    cells = gs.required_cells()
    assert len(cells) == len(set(cells))
    count = Counter(c[0] for c in cells)
    assert count["a"] == 4096 and count["b"] == 64 and count["c"] == 96 and count["f_run"] == 34 * 16
    assert count["d_in"] == count["d_seam"] == 16 and count["d_zero"] == 32 and count["d_total"] == 8
    assert count["e_first"] == count["e_last"] == 30 and count["h"] == 6


def test_batch_sizes():
    """the one-launch forms take every batch but n = 2049; class a's batches
    are its only large ones"""
    for b in gs.all_batches():
        assert len(b.expected) == b.total > 0 and int(b.B[-1]) == b.total
        assert len(b) <= 2048 or b.name == "n2049"
        assert b.total <= (9 << 20) if b.name[0] == "a" else b.total < (2 << 20), b.name
        so, ln = b.descs["payload_off"].astype(np.int64), b.descs["payload_len"].astype(np.int64)
        assert np.all(so + ln <= len(b.src))
        o = np.argsort(so, kind="stable")                          # the sources do not overlap
        ne = o[ln[o] > 0]
        assert np.all(so[ne][1:] >= (so + ln)[ne][:-1]), b.name
    assert sorted(len(b) for b in gs.get_batch("h")) == list(gs.H_COUNTS)


def test_class_a_is_a_chain():
    """every region of a class a batch but its short head is big: each is the
    right side of one seam and the left side of the next"""
    for q, b in enumerate(gs.get_batch("a")):
        assert len(b) <= 2048 and np.all(b.descs["payload_len"][1:] >= gs.BIG)
        got = gs.classify(b.descs[:1026], len(b.src), b.skew)
        assert sum(v for c, v in got.items() if c[0] == "a") == 1024 and sum(c[0] == "a" for c in got) == 1024
        assert {c[1] for c in got if c[0] == "a"} == set(range(4 * q, 4 * q + 4))


def test_class_c_again_behind_4_mib():
    """the last class a batch ends in class c's seams, all of them past the
    first 64 units of every wave of a one-workgroup grid (512 units at 512
    threads)"""
    b = gs.get_batch("a")[3]
    late = {c for c, lo, _ in gs.classify_events(b.descs, len(b.src), b.skew) if lo >= 4 << 20}
    missing = [c for c in gs.required_cells() if c[0] in ("c", "c_unit") and c not in late]
    assert not missing, missing


def test_builder_places_seams_shifts_and_sources():
    lay = gs.Layout(7, lead=0, tail=0)
    lay.add(300, mis=0)
    lay.next_at(4090, shift=9)
    lay.next_mod16(5, shift=0)
    lay.add(0)
    lay.add(33, gap=0)
    lay.add(12, mis=13)
    b = lay.build()
    d, B = b.descs, b.B.astype(np.int64)
    assert list(d["payload_len"][[0, 3, 4, 5]]) == [300, 0, 33, 12]
    assert int(d["payload_off"][0]) == 0                                   # lead = 0: src's first byte
    assert B[2] % gs.UNIT == 4090 and B[2] - B[1] >= gs.BIG
    assert B[3] % 16 == 5 and gs.BIG <= B[3] - B[2] < gs.BIG + 16
    assert (int(d["payload_off"][1]) - B[1]) % 16 == 9 and (int(d["payload_off"][2]) - B[2]) % 16 == 0
    assert int(d["payload_off"][4]) == int(d["payload_off"][2]) + int(d["payload_len"][2])   # adjacent, no gap
    assert int(d["payload_off"][5]) % 16 == 13
    assert int(d["payload_off"][5]) + 12 == len(b.src)                     # tail = 0: src's last byte
    assert b.total == 300 + (B[3] - B[1]) + 33 + 12 == len(b.expected)
    # a view 7 bytes into its tensor: the shift counts from the real address
    lay = gs.Layout(8, skew=7)
    lay.add(100, shift=4)
    lay.add(5000, shift=0)
    b = lay.build()
    assert (7 + int(b.descs["payload_off"][0])) % 16 == 4 and (7 + int(b.descs["payload_off"][1]) - 100) % 16 == 0
    # permuted sources: the same destination order, other source order
    lay = gs.Layout(9, order="perm")
    for k in range(40):
        lay.add(10 + k)
    b = lay.build()
    assert list(b.descs["payload_len"]) == list(range(10, 50)) and (np.diff(b.descs["payload_off"].astype(np.int64)) < 0).any()


def test_classify_hand_written_layout():
    d = np.zeros(4, dtype=gs.FRAME_DESC)
    # B = 0, 3, 4103, 8208, 8208: a tiny first region, a seam of two big regions at 4103 (chunk 0 of unit 1,
    # position 7), one zero-length region after the last byte
    d["payload_len"] = [3, 4100, 4105, 0]
    d["payload_off"] = [14, 32 + 5, 5000 + 0, 0]
    d["phase"] = [0, 1, 2, 0]
    got = gs.classify(d, src_len=5000 + 4105)
    assert got[("a", 7, (37 - 3) % 16, (5000 - 4103) % 16)] == 1 and sum(c[0] == "a" for c in got) == 1
    assert got[("b", 4103 % 4, (4100 + 1) % 4, 2)] == 1
    assert got[("e_first", 14, 1)] == 1 and got[("d_zero", 0, 1)] == 1 and got[("g_end",)] == 1
    assert not any(c[0] in ("c", "f_run", "d_in", "d_seam", "g_src0", "g_perm", "h") for c in got)


def test_describe_byte_names_the_layout():
    b = gs.get_batch("bc")[0]
    B = b.B.astype(np.int64)
    i = next(i for i in range(1, len(b)) if B[i] % gs.UNIT == 16 * 63 + 8)
    s = gs.describe_byte(b.descs, int(B[i]) + 1)
    assert f"region {i} (byte 1 of {int(b.descs['payload_len'][i])}" in s
    assert f"offset {16 * 63 + 9} (chunk 63, lane 63, holds 2 regions), offset 9 in its chunk" in s
    assert "('c', 63, 8, " in s and "('a', 8, " in s


def test_expected_equals_the_oracle():
    """the numpy restatement against orc_ws_mask_fast with RotateR(key, 8 *
    phase), region by region (as test_gpu_onelaunch.py computes it); every
    region of every batch"""
    rot = orc.orc().orc_rotr32
    for b in gs.all_batches():
        exp = np.empty(b.total, dtype=np.uint8)
        w = 0
        for o, n, k, ph in b.descs.tolist():
            seg = b.src[o:o + n].copy()
            orc.orc_mask("ws_mask_fast", seg, rot(k, 8 * ph))
            exp[w:w + n] = seg
            w += n
        assert w == b.total and np.array_equal(exp, b.expected), b.name
