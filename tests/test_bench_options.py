"""bench.py's run options on the CPU: a plain run asks for no extras (--full is
off by default), and --dump-outputs writes float64 .npy files whose sample of
a large field is the same from call to call and stays under the size cap."""
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def test_plain_run_has_no_extras():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 3)
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"


def test_dump_outputs_files(tmp_path):
    res = types.SimpleNamespace(iterations=12, residual=0.25, phi_norm=4.0)
    small = torch.arange(1000, dtype=torch.float64) * 0.5
    n = 4 * bench.DUMP_MAX + 12345
    big = torch.arange(n, dtype=torch.float64)
    rt = {"world": 1, "rank": 0}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), rt, res, {"small": small, "big": big, "big2": -big})
    out = {f: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(out) == ["big.npy", "big2.npy", "cg_scalars.npy", "small.npy"]
    assert all(v.dtype == np.float64 for v in out.values())
    assert np.array_equal(out["small.npy"], small.numpy())
    assert np.array_equal(out["cg_scalars.npy"], [12.0, 0.25, 4.0])
    # the sample: DUMP_MAX values at sorted in-range indices (big holds its own index), the same
    # indices for every field of that length and in every call
    idx = out["big.npy"]
    assert idx.shape == (bench.DUMP_MAX,) and np.all(np.diff(idx) >= 0) and 0 <= idx[0] and idx[-1] < n
    # drawn with replacement from n ~ 4 K values: 4 (1 - exp(-1/4)) = 0.885 of them distinct
    assert len(np.unique(idx)) > 0.8 * bench.DUMP_MAX
    assert np.array_equal(out["big2.npy"], -idx)
    assert np.array_equal(np.load(tmp_path / "b" / "big.npy"), idx)
    # two sampled fields + scalars: far below the 64 MB a dump may take
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in out) < 64e6


def test_dump_outputs_names_shards(tmp_path):
    res = types.SimpleNamespace(iterations=1, residual=0.0, phi_norm=1.0)
    bench.dump_outputs(str(tmp_path), {"world": 2, "rank": 1}, res, {"cg_x": torch.zeros(8, dtype=torch.float64)})
    assert sorted(os.listdir(tmp_path)) == ["cg_scalars_shard1.npy", "cg_x_shard1.npy"]
