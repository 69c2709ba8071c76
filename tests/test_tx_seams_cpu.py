"""The seam sweep's own guard (no GPU): the batches test_gpu_tx_seams.py runs
contain every cell of the class table of tx_seams.py, and the builder's
expected bytes decode back to the payloads it placed.

The coverage test is what keeps the sweep from covering less as someone edits
it: no sampling, no allowance for a missing cell.
"""
from collections import Counter

import numpy as np
import pytest

import orc
import tx_seams as ts


def test_every_class_cell_is_covered():
    got = Counter()
    for b in ts.all_batches():
        got.update(ts.classify(b.descs))
    missing = [c for c in ts.required_cells() if got[c] < 1]
    assert not missing, f"{len(missing)} cells without a batch: {missing}"


def test_required_cells_table():
    cells = ts.required_cells()
    assert len(cells) == len(set(cells))
    assert sum(c[0] == "a" for c in cells) == 96 and sum(c[0] == "b" for c in cells) == 38
    assert sum(c[0] == "c" for c in cells) == 48


@pytest.mark.parametrize("n", ts.J_COUNTS)
def test_frame_count_batches(n):
    b = ts.get_batch(f"n{n}")
    assert len(b) == n and int(b.descs["len"].max()) <= 40


def test_span_batch_geometry():
    """At 8 frames per span every span ends off chunk alignment, and each span
    after a group's starts with 2-byte frames."""
    b = ts.get_batch("spans")
    ends = b.offs[8::8].astype(np.int64)
    assert len(ends) >= 90 and np.all(ends & 15 != 0)
    assert {int(x) & 15 for x in ends[0::3]} == set(range(1, 16))
    for g in range(0, len(b) - 24, 24):
        assert np.all(b.descs["len"][g + 8:g + 24] == 0) and not b.descs["masked"][g + 8:g + 24].any()


def test_builder_places_headers_and_sources():
    lay = ts.Layout(7)
    lay.add(300, masked=1, mis=5)
    lay.next_at(4090, masked=0, shift=9)
    lay.add_to(lay.pos + 70000, masked=1, shift=0)
    with pytest.raises(ValueError):
        lay.add_to(lay.pos + 128, masked=0)           # no unmasked frame has 128 bytes
    b = lay.build()
    assert int(b.descs["src_off"][0]) % 16 == 5
    assert int(b.offs[2]) % ts.UNIT == 4090 and int(b.offs[3]) - int(b.offs[2]) == 70000
    assert (int(b.descs["src_off"][1]) - (int(b.offs[1]) + 4)) % 16 == 9
    assert (int(b.descs["src_off"][2]) - (int(b.offs[2]) + 14)) % 16 == 0
    assert b.total == len(b.expected)
    # payload ranges in the source do not overlap
    so, ln = b.descs["src_off"].astype(np.int64), b.descs["len"].astype(np.int64)
    assert np.all(so[1:] >= so[:-1] + ln[:-1]) and so[-1] + ln[-1] <= len(b.src)


def test_describe_byte_names_the_layout():
    b = ts.get_batch("efi")
    i = next(i for i in range(len(b)) if b.offs[i] % ts.UNIT == 0 and i and b.offs[i + 1] - b.offs[i] == 1024)
    s = ts.describe_byte(b.descs, int(b.offs[i + 1]) + 1)
    assert f"frame {i + 1} (header byte 1" in s and "offset 1025 (chunk 64, lane 0" in s and "('e', 0, 1, 0)" in s


def _check_decodes(b):
    """Every maximal run of masked frames, as a client-to-server stream."""
    d, n, i = b.descs, len(b), 0
    while i < n:
        if not d["masked"][i]:                       # a server frame: the payload as it is, after its header
            so, ln, e = int(d["src_off"][i]), int(d["len"][i]), int(b.offs[i + 1])
            assert e - ln - int(b.offs[i]) == ts.hdr_len(ln, 0)
            assert np.array_equal(b.expected[e - ln:e], b.src[so:so + ln]), (b.name, i)
            i += 1
            continue
        j = i
        while j < n and d["masked"][j]:
            j += 1
        buf = b.expected[int(b.offs[i]):int(b.offs[j])].copy()
        ret, fr, _, cons = orc.orc_decode_stream(buf, frames_cap=j - i)
        assert ret == 0 and len(fr) == j - i and cons == len(buf), (b.name, i, ret)
        rel = (b.offs[i:j] - b.offs[i]).astype(np.uint64)
        assert np.array_equal(fr["hdr_off"], rel) and np.array_equal(fr["payload_len"], d["len"][i:j])
        assert np.array_equal(fr["key"], d["key"][i:j]) and np.array_equal(fr["opcode"], d["opcode"][i:j])
        assert np.array_equal(fr["fin"], d["fin"][i:j])
        for k in range(i, j):
            p = int(rel[k - i]) + int(fr["hdr_len"][k - i])
            so, ln = int(d["src_off"][k]), int(d["len"][k])
            assert np.array_equal(buf[p:p + ln], b.src[so:so + ln]), (b.name, k)
        i = j


def test_expected_bytes_decode_back():
    for b in ts.all_batches():
        assert len(b.expected) == b.total
        _check_decodes(b)
