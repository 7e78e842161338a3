"""GPU: a plain `bench.py` run times exactly the steps it is asked for, prints the headline line without the `--full` legs, and
`--dump-outputs` writes what its last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.mark.gpu
def test_plain_run_times_the_steps_asked_and_dumps_the_last_ones_outputs(tmp_path):
    out = tmp_path / "outputs"
    env = {k: v for k, v in os.environ.items() if k != "TPGSR_CONV_PREC"}      # the headline policy, not the suite's pinned one
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "img/s" and line["higher_is_better"] is True and line["dtype"] == "bf16x2"
    assert not {"roofline", "step_roofline", "alt_precision", "eval", "tpg_opt", "module_api", "cpu_baseline"} & set(line)
    got = {p.name[:-4]: np.load(p) for p in out.iterdir()}
    assert set(got) == {"loss", "sr", "prior", "params", "grads", "bn_buffers"}
    assert sum(a.nbytes for a in got.values()) <= 64_000_000
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert got["loss"].shape == () and abs(float(got["loss"]) - line["final_loss"]) <= 1e-5 * max(1.0, abs(line["final_loss"]))
    assert got["sr"].shape == (48, 4, 32, 128) and got["prior"].shape == (48, 26, 37)
    assert np.allclose(got["prior"].sum(-1), 1.0, atol=1e-4)         # softmax over the 37 classes
