"""GPU parity: fws_gpu_encode_frames on the deterministic seam layouts of
tx_seams.py, through every form of the kernel, bit-exact against the oracle's
orc_tx_frame.

Where test_gpu_tx.py draws random batches, these batches are built so that
every cell of the class table (tx_seams.py: CLASS TABLE; test_tx_seams_cpu.py
asserts the coverage) occurs: headers of every length at every offset of a
16-B chunk, across and at 4 KiB unit boundaries, two seam chunks in one lane,
tiny and empty frames at unit starts, every batch end mod 16, the frame counts
at the plan's edges. A mismatch is reported by layout: the frame, the offset
in its unit and chunk, and the classes of that chunk.

Every call is also checked for: *dev_out_len == total; 64 B before and after
the output (and everything from total to out_cap) untouched; the source and
the descriptors unchanged.
"""
import numpy as np
import pytest
import torch

import tx_seams as ts
from flashws_amd import gpu
from test_gpu_tx import TX_FORMS

pytestmark = pytest.mark.gpu

FORMS = dict(TX_FORMS, plan_w4=0)          # + k_tx_encode, the compiler's 4 waves per SIMD
GUARD, FILL = 64, 0xEE


@pytest.fixture(autouse=True, params=list(FORMS))
def tx_form(request):
    """every test runs on each form of fws_gpu_encode_frames (test_gpu_tx.py's
    six and plan_w4); a test parametrized on tx_form (indirect) runs on the
    forms it names"""
    from flashws_amd._lib import lib
    old = lib().fws_internal_set_tx_one(2 if request.param == "one" else 0, 0)
    old_w = lib().fws_internal_set_tx_w5(FORMS[request.param])
    yield request.param
    lib().fws_internal_set_tx_one(old, 0)
    lib().fws_internal_set_tx_w5(old_w)


def report(b, got, exp):
    diff = np.flatnonzero(got != exp)
    chunks = np.unique(diff // 16)
    lines = [f"batch {b.name} ({len(b)} frames, {b.total} B): {len(diff)} bytes differ in {len(chunks)} chunks"]
    for c in chunks[:4]:
        x = int(diff[np.searchsorted(diff, c * 16)])
        lines.append(f"  {ts.describe_byte(b.descs, x)}; got {got[x]:#04x}, expected {exp[x]:#04x}")
    return "\n".join(lines)


def run_batch(ctx, cuda, b, out_cap=None):
    """Encode b into a tensor of out_cap bytes (default: exactly total) that
    lies GUARD bytes into a larger filled one, and check everything."""
    cap = b.total if out_cap is None else out_cap
    assert cap >= b.total
    buf = torch.full((GUARD + cap + GUARD,), FILL, dtype=torch.uint8, device=cuda)
    out = buf[GUARD:GUARD + cap]
    assert out.data_ptr() % 16 == 0                                   # the ABI's alignment
    dsrc = torch.from_numpy(b.src.copy()).to(cuda)
    dd = torch.from_numpy(b.descs.view(np.uint8).copy()).to(cuda)
    out_len = torch.full((1,), -7, dtype=torch.int64, device=cuda)
    gpu.encode_frames(ctx, out, dsrc, dd, len(b), out_len=out_len)
    torch.cuda.synchronize()
    assert int(out_len.cpu().item()) == b.total, b.name
    exp = torch.from_numpy(b.expected.copy()).to(cuda)
    if not torch.equal(out[:b.total], exp):
        pytest.fail(report(b, out[:b.total].cpu().numpy(), b.expected), pytrace=False)
    assert bool((buf[:GUARD] == FILL).all()), f"{b.name}: bytes before dev_out written"
    assert bool((buf[GUARD + b.total:] == FILL).all()), f"{b.name}: bytes at or past the total written"
    assert np.array_equal(dsrc.cpu().numpy(), b.src), f"{b.name}: the source changed"
    assert dd.cpu().numpy().tobytes() == b.descs.tobytes(), f"{b.name}: the descriptors changed"


@pytest.mark.parametrize("name", list(ts.SEAM_BATCHES))
def test_seam_batch(ctx, cuda, name):
    """classes a-d (abcd), e / f / i (efi), g (g0, g1), k, the span batch"""
    run_batch(ctx, cuda, ts.get_batch(name))


@pytest.mark.parametrize("n", ts.J_COUNTS)
def test_frame_counts(ctx, cuda, n):
    """class j: the frame counts at which the plan forms take another path"""
    run_batch(ctx, cuda, ts.get_batch(f"n{n}"))


def test_batch_ends(ctx, cuda):
    """class h, a small last / first frame at every start mod 16, a tiny first
    frame: many tiny batches, one call each"""
    for b in ts.get_batch("ends"):
        run_batch(ctx, cuda, b)


ONE_BATCHES = ["g0", "g1", "spans"] + [f"n{n}" for n in ts.J_COUNTS]


@pytest.mark.parametrize("tx_form", ["one"], indirect=True)
@pytest.mark.parametrize("name", ONE_BATCHES)
@pytest.mark.parametrize("mode", ["F8", "span4", "span32"])
def test_one_launch_spans(ctx, cuda, tx_form, name, mode):
    """k_tx_one away from its usual 248 frames per workgroup: 8 (an out_cap of
    8 KiB per frame, the output really that large) and spans of 4 and 32 KiB.
    In the span batch at F = 8 every span ends off chunk alignment and the
    next starts with 2-byte frames, the case the look-ahead of 8 frames is for."""
    from flashws_amd._lib import lib
    b = ts.get_batch(name)
    try:
        if mode == "F8":
            run_batch(ctx, cuda, b, out_cap=max(b.total, 8192 * len(b)))
        else:
            lib().fws_internal_set_tx_one(2, int(mode[4:]))
            run_batch(ctx, cuda, b)
    finally:
        lib().fws_internal_set_tx_one(2, 64)


@pytest.mark.parametrize("tx_form", ["plan", "plan_dpp", "plan_sr"], indirect=True)
@pytest.mark.parametrize("blocks", [1, 3])
def test_grid_cap(ctx, cuda, tx_form, blocks):
    """a capped grid: each wave walks many units (tx_encode_body's grid-stride
    loop, every unit after the first found by the owner search)"""
    from flashws_amd._lib import lib
    lib().fws_internal_set_tx_blocks(blocks)
    try:
        run_batch(ctx, cuda, ts.get_batch("abcd"))
    finally:
        lib().fws_internal_set_tx_blocks(0)
