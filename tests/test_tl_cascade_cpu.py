"""CPU: the `_TL` baseline backbones in the fused cascade step through the host layers -- plan recording in dry-run mode
(TPGSR_PLAN_DRYRUN=1, the pattern of tests/test_hd64_cpu.py) for all four backbones, the image-criterion switch, the refusals, the C ABI
of the new entry points and the committed fixtures."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

BACKBONES = ("srresnet_tl", "srcnn_tl", "vdsr_tl", "rdn_tl")

RECORD = r'''
import json, sys, torch
sys.path.insert(0, %(root)r)
from tpgsr_amd import kernels as K
assert K.DRYRUN
from tpgsr_amd.engine_functional import FunctionalSREngine
from tpgsr_amd.interfaces.super_resolution import TPGSRTrainStep
from tpgsr_amd.model import rdn, srcnn, srresnet, vdsr
from tpgsr_amd.model.crnn import crnn

MAKE = {"srresnet_tl": lambda: srresnet.SRResNet_TL(scale_factor=2, width=128, height=32, STN=False, mask=True),
        "srcnn_tl": lambda: srcnn.SRCNN_TL(scale_factor=2, width=128, height=32, STN=False),
        "vdsr_tl": lambda: vdsr.VDSR_TL(scale_factor=2, width=128, height=32, STN=False),
        "rdn_tl": lambda: rdn.RDN_TL(scale_factor=2)}
CRIT = {"srresnet_tl": "mse", "srcnn_tl": "mse", "vdsr_tl": "mse", "rdn_tl": "l1"}

# every launch a dry run makes outside a recording passes the wrapper's check against the C-ABI signature (kernels._launch); the names
# of those launches are collected here
direct = []
_launch = K._launch
def spy(name, *a):
    if K._REC is None:
        direct.append(name)
    return _launch(name, *a)
K._launch = spy

out = {}
torch.manual_seed(0)
for name, make in MAKE.items():
    del direct[:]
    net = make().train()
    stu, teacher = crnn.CRNN(32, 1, 37, 256).train(), crnn.CRNN(32, 1, 37, 256).eval()
    ts = TPGSRTrainStep([net], [stu], teacher, stu_iter=1, image_crit=CRIT[name], precision="x3")
    loss = ts.step(torch.rand(4, 4, 16, 64), torch.rand(4, 4, 32, 128))
    eng = net._engine()
    assert isinstance(eng, FunctionalSREngine) and eng.record and tuple(loss.shape) == ()
    assert tuple(ts.last_sr.shape) == (4, 4, 32, 128)
    (key, pl), = eng._plans.items()
    for p in (pl["fwd"], pl["bwd"]):
        p.run()                                   # the native executor checks entry point and argument count of every op
    a, b = ts.pool.ranges[id(net)]
    out[name] = dict(key=[str(k) for k in key], fwd=[o[0] for o in pl["fwd"].ops], bwd=[o[0] for o in pl["bwd"].ops], direct=list(direct),
                     dprior=list(pl["dprior"].shape), pooled=bool(eng.arena.external is not None and b - a == eng.arena.numel),
                     sunk=all(p.grad is not None for p in net.parameters()))

def refused(**kw):
    net = MAKE["srcnn_tl"]().train()
    stu, teacher = crnn.CRNN(32, 1, 37, 256).train(), crnn.CRNN(32, 1, 37, 256).eval()
    try:
        TPGSRTrainStep([net], [stu], teacher, **kw)
    except Exception as e:
        return [type(e).__name__, str(e)]
    return None

out["unknown_crit"] = refused(image_crit="charbonnier")
out["collective"] = refused(force_collectives=True, image_crit="mse")
out["world2"] = refused(world_size=2, image_crit="mse")
print("RESULT " + json.dumps(out))
'''


@pytest.fixture(scope="module")
def rec():
    env = dict(os.environ, TPGSR_PLAN_DRYRUN="1")
    for k in [k for k in env if k.startswith("TPGSR_") and k != "TPGSR_PLAN_DRYRUN"]:
        del env[k]
    r = subprocess.run([sys.executable, "-c", RECORD % dict(root=ROOT)], capture_output=True, text=True, env=env, timeout=550)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


@pytest.mark.timeout(600)
@pytest.mark.parametrize("name", BACKBONES)
def test_tl_backbone_records_forward_and_backward_plans_without_gpu(rec, name):
    r = rec[name]
    assert r["key"][0] == "(4, 4, 16, 64)" and r["key"][1:] == ["True", "0", "x3"]
    assert len(r["fwd"]) > 40 and len(r["bwd"]) > 40
    assert r["dprior"] == [4, 37, 1, 26] and r["pooled"] and r["sunk"]
    # the text-prior map has 3 to 6 consumers in every backbone: ONE n-way gradient sum; and the slab reduces are one batched program
    assert r["bwd"].count("tpgsr_add_n") == 1
    assert r["bwd"].count("tpgsr_wgrad_reduce_program") == 1 and "tpgsr_wgrad_reduce" not in r["bwd"]
    assert "fork" in r["bwd"] and r["bwd"][-1] == "join"            # weight gradients on their own stream, joined at the end
    assert "join" not in r["fwd"]


def test_l1_criterion_records_the_new_entry_points(rec):
    assert "tpgsr_l1_loss_fwd" in rec["rdn_tl"]["direct"] and "tpgsr_l1_loss_bwd" in rec["rdn_tl"]["direct"]
    assert "tpgsr_image_loss_fwd" not in rec["rdn_tl"]["direct"] and "tpgsr_image_loss_bwd" not in rec["rdn_tl"]["direct"]
    assert "tpgsr_image_loss_finalize" in rec["rdn_tl"]["direct"]
    for name in ("srresnet_tl", "srcnn_tl", "vdsr_tl"):      # "mse": the image-loss kernels
        assert "tpgsr_image_loss_fwd" in rec[name]["direct"] and "tpgsr_l1_loss_fwd" not in rec[name]["direct"]


def test_unknown_image_crit_is_refused(rec):
    assert rec["unknown_crit"] and rec["unknown_crit"][0] == "ValueError" and "charbonnier" in rec["unknown_crit"][1]


def test_gradient_exchange_with_a_functional_sr_engine_is_refused(rec):
    for k in ("collective", "world2"):
        assert rec[k] and rec[k][0] == "NotImplementedError" and "SRCNN_TL" in rec[k][1], rec[k]


def test_new_entry_points_are_declared_bound_and_registered():
    from tpgsr_amd import _lib
    header = open(os.path.join(ROOT, "include", "tpgsr_hip.h")).read()
    plan = open(os.path.join(ROOT, "tpgsr_amd", "csrc", "plan.cpp")).read()
    for sym in ("tpgsr_add_n", "tpgsr_l1_loss_fwd", "tpgsr_l1_loss_bwd"):
        assert sym in _lib.EXPORTED_SYMBOLS
        assert re.search(r"\bint\s+%s\s*\(" % sym, header), sym
        assert "TPGSR_REG(%s)" % sym in plan, sym


@pytest.mark.parametrize("name", BACKBONES + ("srresnet_tl_s2",))
def test_cascade_fixtures_load_and_are_finite(name):
    path = os.path.join(GOLD, f"train_tl_{name}.npz")
    assert os.path.getsize(path) < (1 << 20)
    t = np.load(path, allow_pickle=False)
    stu_iter = 2 if name.endswith("_s2") else 1
    assert t["loss"].shape == (2,) and t["gnorm"].shape == (2,) and t["stu_gnorm"].shape == (2, stu_iter)
    keys = ["loss", "gnorm", "stu_gnorm", "sr_grad_norms", "sr_grad_heads"] + [f"stu{i}_grad_{k}" for i in range(stu_iter) for k in ("norms", "heads")]
    if stu_iter == 1:
        keys.append("sr_step0")
        assert t["sr_step0"].shape == (4, 4, 32, 128) and t["prior_argmax_step0"].shape == (26, 4)
    for k in keys:
        assert np.isfinite(t[k]).all() and t[k].size, k
    assert (t["loss"] > 0).all() and (t["gnorm"] > 0).all() and (t["sr_grad_norms"] > 0).all()
    assert len(t["sr_grad_names"]) == len(t["sr_grad_norms"]) == len(t["sr_grad_heads"])
