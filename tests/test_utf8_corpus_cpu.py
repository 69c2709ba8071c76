"""The UTF-8 conformance corpus (utf8_corpus.py) on the CPU: its counts, its
seam sequences, and the C oracle's orc_utf8_valid pinned to Python's strict
decoder on all of it -- the older GPU tests lean on that oracle."""
import numpy as np

import orc
import utf8_corpus as uc


def test_corpus_e_counts():
    e = uc.corpus_e()
    assert len(e) == 411393 and int(e.ok.sum()) == 20341
    table = {0: (1, 0), 1: (128, 128), 2: (18304, 47232), 3: (236, 13588), 4: (1672, 330104)}
    for n, (well, ill) in table.items():
        m = e.lens == n
        assert (int((e.ok & m).sum()), int((~e.ok & m).sum())) == (well, ill), n
    assert len(uc.B24) == 24 == len(set(uc.B24)) and len(uc.B16) == 16 == len(set(uc.B16))
    # no string twice; the lengths mix along the buffer (a fixed permutation, not sorted by length)
    packed = e.data.view("<u4").reshape(-1).astype(np.int64) * 8 + e.lens
    assert len(np.unique(packed)) == len(e)
    assert len(set(e.lens[:64].tolist())) >= 3
    again = uc._build([(e.data, e.lens)], seed=None)
    assert np.array_equal(again.ok, e.ok)
    assert e.string(int(np.nonzero(e.lens == 0)[0][0])) == b""


def test_corpus_e16_counts():
    c = uc.corpus_e16()
    assert len(c) == 256 + 4096 + 65536
    assert [int((c.lens == n).sum()) for n in (2, 3, 4)] == [256, 4096, 65536]
    cuts = sum(int((c.lens == n).sum()) * (n - 1) for n in (2, 3, 4))
    assert cuts == 205056


def test_oracle_equals_python_on_the_corpus():
    for c in (uc.corpus_e(), uc.corpus_e16()):
        raw = c.data.tobytes()
        got = np.fromiter((orc.orc_utf8_valid(raw[4 * i:4 * i + int(n)]) for i, n in enumerate(c.lens)), dtype=bool,
                          count=len(c))
        bad = np.nonzero(got != c.ok)[0]
        assert bad.size == 0, [c.string(int(i)).hex() for i in bad[:8]]
    wrong = []
    for s in uc.seq_s():
        for before, after in ((0, 0), (0, 31), (31, 0), (29, 33), (1, 2)):
            body, ok = uc.s_case(before, s, after)
            if orc.orc_utf8_valid(body) != ok:
                wrong.append((s.hex(), before, after))
    assert not wrong, wrong[:8]


def test_seam_sequences():
    v, p, i, s = uc.seq_v(), uc.seq_p(), uc.seq_i(), uc.seq_s()
    assert [x.hex() for x in v] == ["c280", "dfbf", "e0a080", "e0bfbf", "e18080", "ecbfbf", "ed8080", "ed9fbf", "ee8080",
                                    "efbfbf", "f0908080", "f0bfbfbf", "f1808080", "f3bfbfbf", "f4808080", "f48fbfbf"]
    assert len(s) == len(set(s)) and set(s) == set(v) | set(p) | set(i)
    assert all(uc.valid(x) for x in v) and not any(uc.valid(x) for x in p + i)
    assert set(p) == {x[:k] for x in v for k in range(1, len(x))} and len(p) == 32
    named = ["c080", "c1bf", "e09fbf", "e08080", "eda080", "edbfbf", "f08fbfbf", "f0808080", "f4908080", "f4bfbfbf",
             "f5808080", "f888808080", "fe", "ff", "80", "bf"]
    assert [x.hex() for x in i[:16]] == named
    for x in v:
        assert x + b"\x80" in i
        for k in range(1, len(x)):
            assert x[:k] + b"\x7f" + x[k + 1:] in i and x[:k] + b"\xc0" + x[k + 1:] in i
    assert len(i) == 16 + sum(2 * (len(x) - 1) for x in v) + 16


def test_filler_keeps_multibyte_characters_at_the_seam():
    for n in range(0, 60):
        for seam in ("left", "right"):
            f = uc.filler(n, seam)
            assert len(f) == n and uc.valid(f)
            if n >= 2:
                assert (f[-1] if seam == "right" else f[0]) >= 0x80
    # an S case is well-formed exactly for the members of V (s_case asserts it), whatever surrounds it
    for s in uc.seq_s():
        assert uc.s_case(40, s, 40)[1] == (s in uc.seq_v())


def test_layouts_and_masking():
    e = uc.corpus_e()
    for shift in range(4):
        buf, offs = uc.layout_slots(e, shift)
        assert int(offs[0]) == 16 + shift and len(buf) % 16 == 0 and len(buf) >= int(offs[-1]) + 4 + 32
        assert set(np.unique(buf[:16 + shift]).tolist()) <= set(uc.HOSTILE)
        assert set(np.unique(buf[int(offs[-1]) + 4:]).tolist()) <= set(uc.HOSTILE)
        for i in (0, 1, 777, len(e) - 1):
            assert buf[offs[i]:offs[i] + e.lens[i]].tobytes() == e.string(i)
            assert set(buf[offs[i] + e.lens[i]:offs[i] + 4].tolist()) <= set(uc.HOSTILE)
    buf, offs = uc.layout_packed(e)
    assert int(offs[0]) == 0 and np.array_equal(np.diff(offs), e.lens[:-1])
    for i in (0, 5, 4242, len(e) - 1):
        assert buf[offs[i]:offs[i] + e.lens[i]].tobytes() == e.string(i)
    # the vectorised masking against the oracle's WSMaskBytesFast restatement, region by region
    rng = np.random.default_rng(9)
    keys = rng.integers(0, 2**32, len(e), dtype=np.uint64).astype(np.uint32)
    phases = rng.integers(0, 4, len(e)).astype(np.uint32)
    masked = uc.mask_strings(buf, e, offs, keys, phases)
    want = buf.copy()
    for i in range(0, len(e), 997):
        key = orc.orc().orc_rotr32(int(keys[i]), 8 * int(phases[i]))
        orc.orc_mask("ws_mask_fast", want, key, int(offs[i]), int(e.lens[i]))
        o, n = int(offs[i]), int(e.lens[i])
        assert masked[o:o + n].tobytes() == want[o:o + n].tobytes(), i
