"""`bench.py --dump-outputs DIR` on the GPU: a plain run (no --full) writes what
the last timed MPI_Reduce_local call left in its inoutbuf, and that is what the
seeded operands give.  32 MiB operands are past the dump's size, so the file
holds the fixed sample (bench.dump_indices); the operands are rebuilt here
from the bench's seed and combined with torch's fp32 add, which rounds once per
element as MPI_SUM does -- the comparison is bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_dump_outputs_is_last_steps_result(cuda, tmp_path):
    import bench
    torch = cuda
    k, w, mib = 5, 3, 32
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(k),
                        "--warmup", str(w), "--mib", str(mib), "--dump-outputs", str(tmp_path)],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["steps"] == k and out["ms_per_step"] > 0 and out["value"] > 0
    assert out["per_rank"][0]["direct_share"] == 1.0
    # a plain run carries none of the --full blocks
    for key in ("sync_variants", "roofline", "config3_sweep", "stream_api", "pcie_inclusive", "cpu_baseline"):
        assert key not in out, key
    got = np.load(tmp_path / "inoutbuf_rank0.npy")
    count = mib * bench.MIB // 4
    idx = bench.dump_indices(count, 1)
    assert got.dtype == np.float32 and got.shape == idx.shape
    # the bench's operands: NPAIRS (inbuf, inoutbuf) pairs from one seeded generator
    g = torch.Generator(device="cuda").manual_seed(0x5EED)
    n = count + bench.SLACK // 4
    pairs = [(torch.rand(n, device="cuda", generator=g) * 2 - 1, torch.rand(n, device="cuda", generator=g) * 2 - 1)
             for _ in range(bench.NPAIRS)]
    last = (w + k - 1) % bench.NPAIRS
    a, b = pairs[last]
    for s in range(w + k):
        if s % bench.NPAIRS == last:
            b = b + a
    want = b[:count][torch.from_numpy(idx).cuda()].cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
