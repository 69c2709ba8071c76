"""GPU parity: fws_gpu_unmask_gather on the deterministic seam layouts of
gather_seams.py, through every form of the kernel, bit-exact against the
restatement that test_gather_seams_cpu.py pins to the oracle's ws_mask_fast.

Where test_gpu_onelaunch.py and the other gather tests draw random layouts,
these batches are built so that every cell of the class table
(gather_seams.py: CLASS TABLE; test_gather_seams_cpu.py asserts the coverage)
occurs: a seam of two large regions at every offset of a 16-B chunk with every
pair of source shifts, every key phase on both sides, seams in the chunks
where lane 63 hands over to the next 1 KiB group and at unit boundaries, every
output end mod 16, tiny regions beside large ones, units of many small and
empty regions, sources at the ends of src and in a misaligned view, the region
counts at the one-launch limit. A mismatch is reported by layout: the region,
the offset in its unit and chunk, and the classes of that chunk.

Every call is also checked for: 64 B before dst and everything from the total
on untouched; the source and the descriptors unchanged.
"""
import numpy as np
import pytest
import torch

import gather_seams as gs
from flashws_amd import _lib, gpu

pytestmark = pytest.mark.gpu

# form -> (fws_internal_set_gather_one, _flat, _dpp, _shape's threads)
FORMS = {"plan_flat": (0, 1, 0, 0), "plan_r05": (0, 0, 0, 0)}
for _dpp, _name in enumerate(("one", "one_dpp", "one_w8", "one_w8_dpp")):
    for _t in (256, 512):
        FORMS[f"{_name}_{_t}"] = (1, 1, _dpp, _t)
PLAN_FORMS = [f for f in FORMS if f.startswith("plan")]
ONE_FORMS = [f for f in FORMS if f.startswith("one")]
GUARD, FILL = 64, 0xEE


@pytest.fixture(autouse=True, params=list(FORMS))
def gather_form(request):
    """every test runs on each form of fws_gpu_unmask_gather: the plan path
    with k_gather_fast<kFlat> (the default) and <false>, and k_gather_one /
    k_gather_one_w8 with and without the DPP neighbour block at 256 and 512
    threads; a test parametrized on gather_form (indirect) runs on the forms it
    names"""
    L = _lib.lib()
    one, flat, dpp, threads = FORMS[request.param]
    old_one = L.fws_internal_set_gather_one(one)
    old_flat = L.fws_internal_set_gather_flat(flat)
    old_dpp = L.fws_internal_set_gather_dpp(dpp)
    try:
        assert L.fws_internal_set_gather_shape(threads, 0) == 0
        yield request.param
    finally:
        L.fws_internal_set_gather_one(old_one)
        L.fws_internal_set_gather_flat(old_flat)
        L.fws_internal_set_gather_dpp(old_dpp)
        L.fws_internal_set_gather_shape(0, 0)      # (returns a status, not the old shape: back to the default)


def report(b, got, exp):
    diff = np.flatnonzero(got != exp)
    chunks = np.unique(diff // 16)
    lines = [f"batch {b.name} ({len(b)} regions, {b.total} B): {len(diff)} bytes differ in {len(chunks)} chunks"]
    for c in chunks[:4]:
        x = int(diff[np.searchsorted(diff, c * 16)])
        lines.append(f"  {gs.describe_byte(b.descs, x, b.skew)}; got {got[x]:#04x}, expected {exp[x]:#04x}")
    return "\n".join(lines)


def run_batch(ctx, cuda, b):
    """Gather b into a 16-B-aligned slice of exactly total bytes that lies
    GUARD bytes into a larger filled tensor, and check everything. src is a
    view b.skew bytes into a 16-B-aligned tensor that ends on a 16-B block, so
    the aligned block of src's last byte lies inside it."""
    buf = torch.full((GUARD + b.total + GUARD,), FILL, dtype=torch.uint8, device=cuda)
    dst = buf[GUARD:GUARD + b.total]
    assert dst.data_ptr() % 16 == 0                                   # the ABI's alignment
    base = torch.zeros((b.skew + len(b.src) + 15) // 16 * 16, dtype=torch.uint8, device=cuda)
    assert base.data_ptr() % 16 == 0
    dsrc = base[b.skew:b.skew + len(b.src)]
    dsrc.copy_(torch.from_numpy(b.src.copy()))
    dd = gpu.descs_to_device(b.descs.copy(), cuda)
    gpu.unmask_gather(ctx, dst, dsrc, dd, len(b))
    torch.cuda.synchronize()
    exp = torch.from_numpy(b.expected.copy()).to(cuda)
    if not torch.equal(dst, exp):
        pytest.fail(report(b, dst.cpu().numpy(), b.expected), pytrace=False)
    assert bool((buf[:GUARD] == FILL).all()), f"{b.name}: bytes before dst written"
    assert bool((buf[GUARD + b.total:] == FILL).all()), f"{b.name}: bytes at or past the total written"
    assert np.array_equal(dsrc.cpu().numpy(), b.src), f"{b.name}: the source changed"
    assert dd.cpu().numpy().tobytes() == b.descs.tobytes(), f"{b.name}: the descriptors changed"


@pytest.mark.parametrize("family", list(gs.FAMILIES))
def test_family(ctx, cuda, family):
    """a: every (seam position, left shift, right shift); bc: key phases, the
    seam's chunk in its unit; d: output ends; e: tiny first / last regions;
    f: units of three or more regions; g: source placement; h: region counts"""
    for b in gs.get_batch(family):
        run_batch(ctx, cuda, b)


@pytest.mark.parametrize("gather_form", PLAN_FORMS, indirect=True)
@pytest.mark.parametrize("family", ["a", "bc"])
def test_small_context(cuda, gather_form, family):
    """classes a - c through a context reserved for 64 KiB: the unit map ends
    after a few units, nearly every unit is found by unit_owner's search and a
    wave walks many units"""
    batches = gs.get_batch(family)
    c = gpu.Ctx(0, max_frames=max(len(b) for b in batches), max_stream_bytes=1 << 16)
    try:
        for b in batches:
            run_batch(c, cuda, b)
    finally:
        c.close()


@pytest.mark.parametrize("gather_form", ONE_FORMS, indirect=True)
@pytest.mark.parametrize("family", ["a", "bc"])
def test_one_workgroup(ctx, cuda, gather_form, family):
    """classes a - c on the one-launch forms at a grid of one workgroup: the
    waves pass their 64th unit and find the later ones by the lds_owner probes
    (class a's batches: from 2 MiB on at 512 threads; the last of them repeats
    class c's seams behind 4 MiB. Batch bc, 1.2 MiB, gets there at 256 threads)"""
    L = _lib.lib()
    old = L.fws_internal_set_gather_blocks(1)
    try:
        for b in gs.get_batch(family):
            if family == "a":
                assert b.total > 2 * 64 * 8 * gs.UNIT                  # half of it past every wave's first 64 units
            run_batch(ctx, cuda, b)
    finally:
        L.fws_internal_set_gather_blocks(old)
