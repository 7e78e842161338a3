"""CPU: bench.py's `--dump-outputs` writer -- float arrays under their names, a large array as a fixed seeded sample, the 64 MB cap -- and
what the benchmarked train steps hand it (dry-run plans: the real shapes without a GPU)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_dump_outputs_writes_float_arrays_and_samples_large_ones(tmp_path):
    n_big = bench.DUMP_MAX_VALUES + 1000
    arrays = {"loss": torch.tensor(1.5), "sr": torch.randn(2, 4, 8, 8), "stat": torch.tensor([1.0, 2.0], dtype=torch.float64),
              "count": torch.tensor([3, 4]), "big": torch.arange(n_big, dtype=torch.float64)}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in arrays}
    assert sorted(os.listdir(tmp_path / "a")) == sorted(f"{n}.npy" for n in arrays)
    assert got["loss"].shape == () and got["loss"].dtype == np.float32 and float(got["loss"]) == 1.5
    assert got["sr"].dtype == np.float32 and np.array_equal(got["sr"], arrays["sr"].numpy())
    assert got["stat"].dtype == np.float64 and got["count"].dtype == np.float32 and got["count"].tolist() == [3.0, 4.0]
    big = got["big"]
    assert big.shape == (bench.DUMP_MAX_VALUES,) and big.dtype == np.float64
    assert (np.diff(big) >= 0).all() and big[0] >= 0 and big[-1] < n_big and (big == np.round(big)).all()
    assert np.array_equal(big, np.load(tmp_path / "b" / "big.npy"))       # same positions on every run


def test_dump_outputs_refuses_more_than_64_mb(tmp_path):
    arrays = {f"x{i}": torch.zeros(bench.DUMP_MAX_VALUES) for i in range(3)}
    with pytest.raises(RuntimeError, match="limit"):
        bench.dump_outputs(str(tmp_path / "d"), arrays)
    assert not (tmp_path / "d").exists()


_SCRIPT = r"""
import json, sys
sys.path.insert(0, %(root)r)
import torch, bench
res = {}
for cfg in ("c3", "c2", "c5"):
    ts, _ = bench.build_step(cfg, torch.device("cpu"))
    lr, hr = bench.synthetic_batch(bench.CONFIGS[cfg]["batch"], 1234, torch.device("cpu"))
    a = bench.train_step_outputs(ts, ts.step(lr, hr))
    res[cfg] = {k: list(v.shape) for k, v in a.items()}
print(json.dumps(res))
"""


def test_train_step_outputs_of_every_config_fit_the_dump():
    env = dict(os.environ, TPGSR_PLAN_DRYRUN="1")
    r = subprocess.run([sys.executable, "-c", _SCRIPT % dict(root=ROOT)], capture_output=True, text=True, env=env, timeout=550)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    for cfg, shapes in res.items():
        B = bench.CONFIGS[cfg]["batch"]
        want = {"loss", "sr", "params", "grads", "bn_buffers"} | ({"prior"} if bench.CONFIGS[cfg]["tl"] else set())
        assert set(shapes) == want, cfg
        assert shapes["loss"] == [] and shapes["sr"] == [B, 4, 32, 128] and shapes["params"] == shapes["grads"]
        if "prior" in shapes:
            assert shapes["prior"] == [B, 26, 37]
        written = sum(min(int(np.prod(s)), bench.DUMP_MAX_VALUES) for s in shapes.values()) * 4
        assert written <= bench.DUMP_MAX_BYTES, (cfg, written)
