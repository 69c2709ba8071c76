"""bench.py as a program on the GPU: a plain run prints the headline line alone,
and --dump-outputs writes what its last timed step computed -- the batch with
its payloads unmasked -- whatever the number of steps and buffers, checked
against the CPU oracle's decode of the same generated batch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import orc
from flashws_amd import gpu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES, PAYLOAD = 300, 1000            # 302,400 wire bytes: the last 4 KiB block is partial


@pytest.fixture(scope="module")
def unmasked():
    import bench
    wire, descs, _ = gpu.config_c2(seed=bench.shard_seed(0), n_frames=FRAMES, payload=PAYLOAD)
    exp = wire.copy()
    ret, frames, _, _ = orc.orc_decode_stream(exp)
    assert ret == 0 and len(frames) == FRAMES and not np.array_equal(exp, wire)
    nb = -(-len(exp) // bench.DUMP_BLOCK)
    return np.concatenate([exp, np.zeros(nb * bench.DUMP_BLOCK - len(exp), dtype=np.uint8)]).reshape(nb, -1)


# the last step's buffer enters the timed steps masked (3 steps over 4 buffers) or
# unmasked (an even number of its calls are timed: 3 over 2, 4 over 1)
@pytest.mark.parametrize("steps,nbuf", [(3, 4), (3, 2), (4, 1)])
def test_plain_run_dumps_the_unmasked_batch(cuda, unmasked, tmp_path, steps, nbuf):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                          "--warmup", "1", "--frames", str(FRAMES), "--payload", str(PAYLOAD), "--nbuf", str(nbuf),
                          "--dump-outputs", str(tmp_path)],
                         cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [json.loads(x) for x in out.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, out.stdout
    rec = lines[0]
    assert rec["steps"] == steps and rec["ms_per_step"] > 0 and rec["unit"] == "GiB/s"
    assert "extra" not in rec and "cpu_baseline" not in rec
    assert rec["outputs_dumped"] == ["block_byte_sums.npy", "block_sample.npy"]
    sums = np.load(tmp_path / "block_byte_sums.npy")
    sample = np.load(tmp_path / "block_sample.npy")
    assert sums.dtype == np.float64 and sample.dtype == np.float32
    assert np.array_equal(sums, unmasked.sum(axis=1))
    assert np.array_equal(sample, unmasked)                # fewer blocks than the sample holds: every block
