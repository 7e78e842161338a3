"""CPU: the prior-free baselines (`--arch srres | rdn | vdsr | bicubic`: SRResNet / RDN / VDSR / BICUBIC) through the host layers -- the
state_dict layouts against the reference's (tests/golden/plain_layouts.json), plan recording in dry-run mode (TPGSR_PLAN_DRYRUN=1, the
pattern of tests/test_tl_cascade_cpu.py) through `SRTrainStep`, the criterion and channel-prefix switches, the refusals, the C ABI of the
new entry point and the committed fixtures."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
sys.path.insert(0, GOLD)

BACKBONES = ("srres", "rdn", "vdsr")


def build(name):
    from tpgsr_amd.model import rdn, srresnet, vdsr
    if name == "srres":
        return srresnet.SRResNet(scale_factor=2, width=128, height=32, STN=False, mask=True)
    if name == "rdn":
        return rdn.RDN(scale_factor=2)
    return vdsr.VDSR(scale_factor=2, width=128, height=32, STN=False)


@pytest.mark.parametrize("name", BACKBONES)
def test_state_dict_layout_equals_the_reference(name):
    from make_golden_next import generic_recipe
    lay = json.load(open(os.path.join(GOLD, "plain_layouts.json")))[name]
    net = build(name)
    assert [(k, list(v.shape)) for k, v in net.state_dict().items()] == [(a, b) for a, b in lay]
    # a checkpoint in the reference's layout (keys and shapes from the fixture alone) loads strictly
    ckpt = generic_recipe({k: torch.empty(s, dtype=torch.int64 if k.endswith("num_batches_tracked") else torch.float32) for k, s in lay}, 7)
    res = net.load_state_dict(ckpt, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in net.state_dict().items():
        assert torch.equal(v, ckpt[k]), k


def test_constructor_signatures_and_refusals():
    import inspect
    from tpgsr_amd.model import bicubic, rdn, srresnet, vdsr
    sig = lambda c: [(p.name, p.default) for p in list(inspect.signature(c.__init__).parameters.values())[1:]]
    assert sig(srresnet.SRResNet) == [("scale_factor", 2), ("STN", False), ("width", 128), ("height", 32), ("mask", False)]
    assert sig(rdn.RDN) == [("nChannel", 3), ("nDenselayer", 6), ("nFeat", 64), ("scale_factor", 2), ("growthRate", 32)]
    assert sig(vdsr.VDSR) == [("scale_factor", 2), ("in_planes", 3), ("width", 32), ("height", 128), ("STN", False)]
    assert sig(bicubic.BICUBIC) == [("scale_factor", 2)]
    with pytest.raises(NotImplementedError):
        srresnet.SRResNet(STN=True)
    with pytest.raises(NotImplementedError):
        srresnet.SRResNet(scale_factor=4)
    assert srresnet.ResidualBlock(64) and rdn.RDB(64, 6, 32) and vdsr.Conv_ReLU_Block()
    # VDSR's initialisation (reference model/vdsr.py:48-51): N(0, sqrt(2 / (k * k * Cout))) on every conv weight
    torch.manual_seed(3)
    w = vdsr.VDSR().residual_layer[0].conv.weight
    assert abs(float(w.detach().std()) -(2.0 / (9 * 64)) ** 0.5) < 0.03 * (2.0 / (9 * 64)) ** 0.5


def test_modules_and_bicubic_have_no_cpu_path():
    from tpgsr_amd.model import bicubic
    for name in BACKBONES:
        with pytest.raises(RuntimeError, match="no CPU|GPU only"):
            build(name)(torch.zeros(1, 4 if name == "srres" else 3, 16, 64))
    with pytest.raises(RuntimeError, match="no CPU|GPU only"):
        bicubic.BICUBIC()(torch.zeros(1, 3, 16, 64))


def test_new_entry_point_is_declared_bound_and_registered():
    from tpgsr_amd import _lib
    header = open(os.path.join(ROOT, "include", "tpgsr_hip.h")).read()
    plan = open(os.path.join(ROOT, "tpgsr_amd", "csrc", "plan.cpp")).read()
    sym = "tpgsr_bicubic_upsample"
    assert sym in _lib.EXPORTED_SYMBOLS
    assert re.search(r"\bint\s+%s\s*\(" % sym, header)
    assert "TPGSR_REG(%s)" % sym in plan
    assert hasattr(_lib.load(), sym)


RECORD = r'''
import json, sys, torch
sys.path.insert(0, %(root)r)
from tpgsr_amd import kernels as K
assert K.DRYRUN
from tpgsr_amd.engine_functional import FunctionalSREngine, PlainSREngine
from tpgsr_amd.interfaces.super_resolution import SRTrainStep, TSRNTrainStep, TextSREvaluator
from tpgsr_amd.model import bicubic, rdn, srresnet, tsrn, vdsr
from tpgsr_amd.model.crnn import crnn
assert SRTrainStep is TSRNTrainStep

MAKE = {"srres": lambda: srresnet.SRResNet(scale_factor=2, width=128, height=32, STN=False, mask=True),
        "rdn": lambda: rdn.RDN(scale_factor=2),
        "vdsr": lambda: vdsr.VDSR(scale_factor=2, width=128, height=32, STN=False)}
KW = {"srres": dict(image_crit="mse"), "rdn": dict(image_crit="l1", channels=3), "vdsr": dict(image_crit="mse", channels=3)}

direct = []          # (name, args) of every launch made outside a recording
_launch = K._launch
def spy(name, *a):
    if K._REC is None:
        direct.append((name, [x for x in a if isinstance(x, int) and not isinstance(x, bool)]))
    return _launch(name, *a)
K._launch = spy

out = {}
torch.manual_seed(0)
for name, make in MAKE.items():
    del direct[:]
    net = make().train()
    ts = SRTrainStep(net, precision="x3", **KW[name])
    loss = ts.step(torch.rand(4, 4, 16, 64), torch.rand(4, 4, 32, 128))
    eng = net._engine()
    assert isinstance(eng, PlainSREngine) and isinstance(eng, FunctionalSREngine) and eng.record and tuple(loss.shape) == ()
    (key, pl), = eng._plans.items()
    for p in (pl["fwd"], pl["bwd"]):
        p.run()                                   # the native executor checks entry point and argument count of every op
    a, b = ts.pool.ranges[id(net)]
    out[name] = dict(key=[str(k) for k in key], fwd=[o[0] for o in pl["fwd"].ops], bwd=[o[0] for o in pl["bwd"].ops],
                     direct=[d[0] for d in direct],      # (arguments 0 and 3 of the strided copy are the two pointers)
                     strided=[d[1][1:3] + d[1][4:] for d in direct if d[0] == "tpgsr_copy_strided"],
                     sr=list(ts.last_sr.shape), pooled=bool(eng.arena.external is not None and b - a == eng.arena.numel),
                     sunk=all(p.grad is not None for p in net.parameters()), has_prior=("prior" in pl or "dprior" in pl))

def refused(make, **kw):
    try:
        SRTrainStep(make().train(), **kw)
    except Exception as e:
        return [type(e).__name__, str(e)]
    return None

out["collective"] = refused(MAKE["srres"], force_collectives=True, image_crit="mse")
out["world2"] = refused(MAKE["rdn"], world_size=2, image_crit="l1", channels=3)
out["unknown_crit"] = refused(MAKE["srres"], image_crit="charbonnier")

def tsrn_names(**kw):
    torch.manual_seed(1)
    del direct[:]
    net = tsrn.TSRN(scale_factor=2, width=128, height=32, STN=True, mask=True).train()
    ts = TSRNTrainStep(net, precision="x3", **kw)
    ts.step(torch.rand(4, 4, 16, 64), torch.rand(4, 4, 32, 128))
    eng = net._engine()
    names = [d[0] for d in direct]
    for attr in ("_plans", "_plan_cache"):
        if hasattr(eng, attr):
            for k, pl in sorted(getattr(eng, attr).items(), key=lambda kv: str(kv[0])):
                for q in (pl.values() if isinstance(pl, dict) else [pl]):
                    if isinstance(q, K.Plan):
                        names += [o[0] for o in q.ops]
    return names

out["tsrn_default"] = tsrn_names()
out["tsrn_explicit"] = tsrn_names(image_crit="image_loss", channels=None)

# the prior-free evaluator pass: no text-prior launches
rec = crnn.CRNN(32, 1, 37, 256).eval()
for name, model, ch in (("srres", MAKE["srres"]().eval(), None), ("rdn", MAKE["rdn"]().eval(), 3), ("bicubic", bicubic.BICUBIC(2), 3)):
    del direct[:]
    ev = TextSREvaluator([model], None, recognizer=rec, channels=ch)
    srs, priors = ev.super_resolve(torch.rand(6, 4, 16, 64))
    out["eval_" + name] = dict(direct=[d[0] for d in direct], sr=list(srs[0].shape), priors=len(priors))
try:
    TextSREvaluator([MAKE["srres"]().train()], None, recognizer=rec).super_resolve(torch.rand(2, 4, 16, 64))
    out["eval_train_mode"] = None
except Exception as e:
    out["eval_train_mode"] = [type(e).__name__, str(e)]
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


PRIOR_LAUNCHES = ("tpgsr_softmax_prior_fwd", "tpgsr_softmax_prior_bwd", "tpgsr_semantic_loss_finalize", "tpgsr_resize_bilinear_fwd",
                  "tpgsr_resize_bilinear_bwd", "tpgsr_dilate2d", "tpgsr_bicubic_gray_fwd")


@pytest.mark.timeout(600)
@pytest.mark.parametrize("name", BACKBONES)
def test_plain_backbone_records_forward_and_backward_plans_without_gpu(rec, name):
    r = rec[name]
    C = 4 if name == "srres" else 3
    assert r["key"][0] == f"(4, {C}, 16, 64)" and r["key"][1:] == ["True", "0", "x3"]
    assert len(r["fwd"]) > 15 and len(r["bwd"]) > 15
    assert r["sr"] == [4, C, 32, 128] and r["pooled"] and r["sunk"] and not r["has_prior"]
    assert r["bwd"].count("tpgsr_wgrad_reduce_program") == 1 and "tpgsr_wgrad_reduce" not in r["bwd"]
    assert "fork" in r["bwd"] and r["bwd"][-1] == "join"            # weight gradients on their own stream, joined at the end
    assert "join" not in r["fwd"]
    for p in PRIOR_LAUNCHES:                                        # no text prior anywhere: neither in the plans nor next to them
        assert p not in r["fwd"] and p not in r["bwd"] and p not in r["direct"], p


def test_criterion_switch_records_the_matching_kernels(rec):
    d = rec["rdn"]["direct"]
    assert "tpgsr_l1_loss_fwd" in d and "tpgsr_l1_loss_bwd" in d and "tpgsr_image_loss_finalize" in d
    assert "tpgsr_image_loss_fwd" not in d and "tpgsr_image_loss_bwd" not in d
    for name in ("srres", "vdsr"):
        d = rec[name]["direct"]
        assert "tpgsr_image_loss_fwd" in d and "tpgsr_image_loss_bwd" in d and "tpgsr_l1_loss_fwd" not in d


def test_channel_prefix_is_a_strided_copy_launch(rec):
    assert rec["srres"]["strided"] == []                            # channels=None: nothing is gathered
    for name in ("rdn", "vdsr"):
        # lr (4, 4, 16, 64) -> (4, 3, 16, 64) and hr (4, 4, 32, 128) -> (4, 3, 32, 128): rows = samples, row = the first 3 planes
        assert rec[name]["strided"] == [[4 * 16 * 64, 0, 3 * 16 * 64, 0, 4, 3 * 16 * 64, 0], [4 * 32 * 128, 0, 3 * 32 * 128, 0, 4, 3 * 32 * 128, 0]]


def test_gradient_exchange_with_a_functional_engine_is_refused(rec):
    assert rec["collective"] and rec["collective"][0] == "NotImplementedError" and "SRResNet" in rec["collective"][1]
    assert rec["world2"] and rec["world2"][0] == "NotImplementedError" and "RDN" in rec["world2"][1]
    assert "gradient exchange (world_size > 1 / force_collectives)" in rec["collective"][1]
    assert rec["unknown_crit"] and rec["unknown_crit"][0] == "ValueError" and "charbonnier" in rec["unknown_crit"][1]


def test_default_tsrn_step_records_the_same_launches(rec):
    assert len(rec["tsrn_default"]) > 100
    assert rec["tsrn_default"] == rec["tsrn_explicit"]
    assert "tpgsr_copy_strided" not in [n for n in rec["tsrn_default"][:8]] and "tpgsr_l1_loss_fwd" not in rec["tsrn_default"]


def test_prior_free_evaluator_pass_runs_no_text_prior_generator(rec):
    for name, C in (("srres", 4), ("rdn", 3), ("bicubic", 3)):
        r = rec["eval_" + name]
        assert r["sr"] == [6, C, 32, 128] and r["priors"] == 0
        for p in PRIOR_LAUNCHES:
            assert p not in r["direct"], (name, p)
    assert rec["eval_bicubic"]["direct"] == ["tpgsr_bicubic_upsample"]
    assert rec["eval_train_mode"] and rec["eval_train_mode"][0] == "RuntimeError" and "eval()" in rec["eval_train_mode"][1]


@pytest.mark.parametrize("name", BACKBONES)
def test_fixtures_load_and_are_finite(name):
    C = 4 if name == "srres" else 3
    g = np.load(os.path.join(GOLD, f"plain_{name}.npz"), allow_pickle=False)
    t = np.load(os.path.join(GOLD, f"train_plain_{name}.npz"), allow_pickle=False)
    for path in (f"plain_{name}.npz", f"train_plain_{name}.npz"):
        assert os.path.getsize(os.path.join(GOLD, path)) < 700 * 1024
    assert g["y"].shape == g["y_eval"].shape == t["sr_step0"].shape == (4, C, 32, 128) and g["y_small"].shape == (2, C, 24, 80)
    assert t["loss"].shape == (2,) and t["gnorm"].shape == (2,) and (t["loss"] > 0).all() and (t["gnorm"] > 0).all()
    for k in ("y", "y_eval", "y_small", "grad_norms", "grad_heads", "running_cat"):
        assert np.isfinite(g[k]).all() and g[k].size, k
    assert len(g["grad_names"]) == len(g["grad_norms"]) == len(g["grad_heads"]) == len(list(build(name).parameters()))
    assert (g["grad_norms"] > 0).all()
    ev = json.load(open(os.path.join(GOLD, "plain_eval.json")))
    assert ev["n"] == 6 and set(ev["strings"]) == {"lr", "hr", "sr_srres", "sr_tsrn", "sr_rdn", "sr_bicubic"}
    assert all(len(v) == 6 for v in ev["strings"].values())
