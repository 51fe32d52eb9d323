"""bench.py --dump-outputs on the GPU: a small run in a child process of its own, its dumped sample checked against the keys it joined."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_dump_outputs_is_the_last_steps_join(gdf, tmp_path):
    import torch
    sys.path.insert(0, ROOT)
    import bench
    npr, nb = 1_000_000, 100_000
    env = {k: v for k, v in os.environ.items() if k != "LIBGDF_AMD_TESTHOOK"}
    run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--probe-rows", str(npr),
                          "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0, run.stderr[-3000:]
    line = json.loads([l for l in run.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["config"]["build_rows_per_gpu"] == nb
    assert "extra" not in line and "cpu_baseline" not in line                    # a plain run: the headline only
    rows, brow, count = (np.load(os.path.join(tmp_path, f"{n}.npy")) for n in ("probe_row", "build_row", "pair_count"))
    assert rows.dtype == brow.dtype == count.dtype == np.float64
    assert count.tolist() == [float(npr)] and line["config"]["out_rows"] == npr
    np.testing.assert_array_equal(rows, np.arange(npr))                          # fewer probe rows than the sample: all of them
    dev = torch.device("cuda", 0)
    build = bench.make_build_keys(nb, 0x5EED0001, dev)
    probe = bench.make_probe_keys(npr, nb, 0x5EED0002, dev)
    b = torch.from_numpy(brow.astype(np.int64)).to(dev)
    assert int(b.min()) >= 0 and int(b.max()) < nb
    assert torch.equal(probe[torch.from_numpy(rows.astype(np.int64)).to(dev)], build[b])
