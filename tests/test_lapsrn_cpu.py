"""CPU: `--arch lapsrn` (LapSRN x2 / x4, L1_Charbonnier_loss) through the host layers -- constructor, state_dict layout against the
reference's (tests/golden/lapsrn_layouts.json), initialisation, refusals, the C ABI of the new entry points, and plan recording in dry-run
mode (TPGSR_PLAN_DRYRUN=1, the pattern of tests/test_plain_baselines_cpu.py) through `SRTrainStep` with the new criterion value and through
the prior-free evaluator pass; the committed fixtures."""
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

NEW_SYMBOLS = ("tpgsr_tconv4s2_expand", "tpgsr_tconv4s2_fold_grad", "tpgsr_tconv4s2_small_fwd", "tpgsr_tconv4s2_small_bwd_data",
               "tpgsr_tconv4s2_small_bwd_weight", "tpgsr_leaky_relu_fwd", "tpgsr_leaky_relu_bwd", "tpgsr_charbonnier_loss_fwd",
               "tpgsr_charbonnier_loss_bwd")


def test_constructor_signature():
    import inspect
    from tpgsr_amd.model import lapsrn
    sig = [(p.name, p.default) for p in list(inspect.signature(lapsrn.LapSRN.__init__).parameters.values())[1:]]
    assert sig == [("scale_factor", 2), ("in_planes", 3), ("STN", False), ("width", 128), ("height", 32)]
    assert lapsrn.L1_Charbonnier_loss().eps == 1e-6
    assert lapsrn.LapSRN(scale_factor=4, width=256, height=64).tps_inputsize == [16, 64]


@pytest.mark.parametrize("scale", [2, 4])
def test_state_dict_layout_equals_the_reference(scale):
    from make_golden_next import generic_recipe
    from tpgsr_amd.model import lapsrn
    lay = json.load(open(os.path.join(GOLD, "lapsrn_layouts.json")))[f"x{scale}"]
    net = lapsrn.LapSRN(scale_factor=scale)
    assert [(k, list(v.shape)) for k, v in net.state_dict().items()] == [(a, b) for a, b in lay]
    keys = [k for k, _ in lay]
    assert keys[:3] == ["conv_input.weight", "convt_I1.weight", "convt_R1.weight"]
    assert [k for k in keys if k.startswith("convt_F2")] == [f"convt_F2.0.cov_block.{i}.weight" for i in range(0, 21, 2)]      # also at x2
    ckpt = generic_recipe({k: torch.empty(s) for k, s in lay}, 7)      # a checkpoint in the reference's layout loads strictly
    res = net.load_state_dict(ckpt, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in net.state_dict().items():
        assert torch.equal(v, ckpt[k]), k


def test_initialisation():
    from tpgsr_amd.model import lapsrn
    torch.manual_seed(5)
    net = lapsrn.LapSRN(scale_factor=4)
    tent = torch.tensor([0.25, 0.75, 0.75, 0.25])
    want = torch.outer(tent, tent)
    tconvs = [net.convt_I1, net.convt_I2, net.convt_F1[0].cov_block[20], net.convt_F2[0].cov_block[20]]
    assert [tuple(m.weight.shape) for m in tconvs] == [(3, 3, 4, 4), (3, 3, 4, 4), (64, 64, 4, 4), (64, 64, 4, 4)]
    for m in tconvs:      # the bilinear filter repeated over both channel axes, exactly
        assert torch.equal(m.weight.detach(), want.expand_as(m.weight))
    assert torch.equal(lapsrn.bilinear_kernel(4), want)
    # convolutions: N(0, sqrt(2 / (k * k * Cout)))
    for w, cout in ((net.convt_F1[0].cov_block[4].weight, 64), (net.conv_input.weight, 64)):
        std = (2.0 / (9 * cout)) ** 0.5
        assert abs(float(w.detach().std()) - std) < 0.06 * std
    assert abs(float(net.convt_R1.weight.detach().std()) - (2.0 / 27) ** 0.5) < 0.15 * (2.0 / 27) ** 0.5      # (1728 samples)


def test_refusals():
    from tpgsr_amd.model import lapsrn
    with pytest.raises(NotImplementedError, match="STN"):
        lapsrn.LapSRN(STN=True)
    for s in (1, 3, 8):
        with pytest.raises(ValueError, match="scale_factor"):
            lapsrn.LapSRN(scale_factor=s)
    with pytest.raises(RuntimeError, match="no CPU|GPU only"):
        lapsrn.LapSRN()(torch.zeros(1, 3, 16, 64))
    with pytest.raises(RuntimeError, match="no CPU|GPU only"):
        lapsrn.L1_Charbonnier_loss()(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4))


def test_new_entry_points_are_declared_bound_and_registered():
    from tpgsr_amd import _lib
    header = open(os.path.join(ROOT, "include", "tpgsr_hip.h")).read()
    plan = open(os.path.join(ROOT, "tpgsr_amd", "csrc", "plan.cpp")).read()
    for sym in NEW_SYMBOLS:
        assert sym in _lib.EXPORTED_SYMBOLS
        assert re.search(r"\bint\s+%s\s*\(" % sym, header)
        assert "TPGSR_REG(%s)" % sym in plan
        assert hasattr(_lib.load(), sym)
    assert len(_lib.ABI_STRUCTS) == 13      # scalar parameters only


def test_form_table_of_the_transposed_convolution():
    from tpgsr_amd import functional as Fh
    assert Fh.tconv_k4s2_form(64, 64) == "subpixel"
    assert Fh.tconv_k4s2_form(3, 3) == Fh.tconv_k4s2_form(4, 4) == Fh.tconv_k4s2_form(2, 3) == "direct"
    assert Fh.tconv_k4s2_form(8, 8) == Fh.tconv_k4s2_form(5, 3) == "dilated"


RECORD = r'''
import json, sys, torch
sys.path.insert(0, %(root)r)
from tpgsr_amd import kernels as K
assert K.DRYRUN
from tpgsr_amd import functional as Fh
from tpgsr_amd.engine_functional import PlainSREngine
from tpgsr_amd.interfaces.super_resolution import SRTrainStep, TextSREvaluator
from tpgsr_amd.model import lapsrn, srresnet
from tpgsr_amd.model.crnn import crnn

direct = []
_launch = K._launch
def spy(name, *a):
    if K._REC is None:
        direct.append(name)
    return _launch(name, *a)
K._launch = spy

def err(f):
    try:
        f()
    except Exception as e:
        return [type(e).__name__, str(e)]
    return None

out = {}
torch.manual_seed(0)
for s in (2, 4):
    del direct[:]
    net = lapsrn.LapSRN(scale_factor=s).train()
    ts = SRTrainStep(net, precision="x3", image_crit="l1_charbonnier", channels=3)
    loss = ts.step(torch.rand(4, 4, 16, 64), torch.rand(4, 4, 16 * s, 64 * s))
    eng = net._engine()
    assert isinstance(eng, PlainSREngine) and eng.record and tuple(loss.shape) == ()
    (key, pl), = eng._plans.items()
    for p in (pl["fwd"], pl["bwd"]):
        p.run()                                   # the native executor checks entry point and argument count of every op
    a, b = ts.pool.ranges[id(net)]
    live = [n for n, p in net.named_parameters() if s == 4 or not n.startswith(("convt_I2", "convt_R2", "convt_F2"))]
    out[str(s)] = dict(key=[str(k) for k in key], fwd=[o[0] for o in pl["fwd"].ops], bwd=[o[0] for o in pl["bwd"].ops], direct=list(direct),
                       sr=list(ts.last_sr.shape), scale=eng.scale, pooled=bool(eng.arena.external is not None and b - a == eng.arena.numel),
                       sunk=all(p.grad is not None for p in net.parameters()), n_live=len(live), has_prior=("prior" in pl or "dprior" in pl),
                       wrong_hr=err(lambda: ts.step(torch.rand(4, 4, 16, 64), torch.rand(4, 4, 8 * s, 32 * s))))
out["srres_scale"] = srresnet.SRResNet()._engine().scale
out["class_scale"] = PlainSREngine.scale

rec = crnn.CRNN(32, 1, 37, 256).eval()
for s in (2, 4):
    del direct[:]
    net = lapsrn.LapSRN(scale_factor=s).eval()
    ev = TextSREvaluator([net], None, recognizer=rec, channels=3)
    srs, priors = ev.super_resolve(torch.rand(6, 4, 16, 64))
    (pl,) = net._engine()._plans.values()
    out["eval_%%d" %% s] = dict(direct=list(direct), sr=list(srs[0].shape), priors=len(priors), plan=[o[0] for o in pl["fwd"].ops])

# the other forms of the functional op, and its refusals
x = torch.rand(2, 3, 5, 8).requires_grad_(True)
w = torch.rand(8, 8, 4, 4).requires_grad_(True)
del direct[:]
y = Fh.conv_transpose2d_k4s2(x, w)
y.sum().backward()
out["dilated_8x8"] = dict(direct=list(direct), y=list(y.shape))
out["bad_form"] = err(lambda: Fh.conv_transpose2d_k4s2(x, w, form="subpixel"))
out["bad_weight"] = err(lambda: Fh.conv_transpose2d_k4s2(x, torch.rand(8, 8, 3, 3)))
out["cin5"] = err(lambda: K.tconv4s2_small_fwd(torch.rand(1, 2, 2, 5), torch.rand(5, 3, 4, 4), 1, 2, 2, 5, 3, torch.rand(1, 4, 4, 3)))
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
@pytest.mark.parametrize("scale", [2, 4])
def test_lapsrn_records_forward_and_backward_plans_without_gpu(rec, scale):
    r = rec[str(scale)]
    n_up = 1 if scale == 2 else 2
    assert r["key"] == ["(4, 3, 16, 64)", "True", "0", "x3"]
    assert r["sr"] == [4, 3, 16 * scale, 64 * scale] and r["pooled"] and r["sunk"] and not r["has_prior"]
    fwd, bwd = r["fwd"], r["bwd"]
    # the 64 -> 64 transposed convolutions take the sub-pixel route: no zero-dilated tensor anywhere, one weight expansion per stage
    assert "tpgsr_dilate2d" not in fwd and "tpgsr_dilate2d" not in bwd and "tpgsr_subsample2d" not in bwd
    assert fwd.count("tpgsr_tconv4s2_expand") == n_up and fwd.count("tpgsr_tconv4s2_small_fwd") == n_up
    assert fwd.count("tpgsr_conv_fwd") == 1 + 12 * n_up and fwd.count("tpgsr_leaky_relu_fwd") == 1 + 11 * n_up
    assert fwd.count("tpgsr_add") == n_up and "join" not in fwd
    # backward: the fold behind its own slab reduce, the image branch's partial sums behind reduce_partials; every other weight gradient
    # in the one batched reduce; the image branch's data gradient only where its input has one (the second stage)
    assert bwd.count("tpgsr_tconv4s2_fold_grad") == bwd.count("tpgsr_wgrad_reduce") == n_up
    for i, name in enumerate(bwd):
        if name == "tpgsr_tconv4s2_fold_grad":
            assert bwd[i - 1] == "tpgsr_wgrad_reduce" and bwd[i - 2] == "tpgsr_conv_wgrad"
        if name == "tpgsr_tconv4s2_small_bwd_weight":
            assert bwd[i + 1] == "tpgsr_reduce_partials"
    assert bwd.count("tpgsr_tconv4s2_small_bwd_weight") == bwd.count("tpgsr_reduce_partials") == n_up
    assert bwd.count("tpgsr_tconv4s2_small_bwd_data") == n_up - 1
    assert bwd.count("tpgsr_wgrad_reduce_program") == 1 and bwd.count("tpgsr_leaky_relu_bwd") == 1 + 11 * n_up
    assert "fork" in bwd and bwd[-1] == "join"
    assert r["n_live"] == (14 if scale == 2 else 27)


def test_l1_charbonnier_records_its_kernels(rec):
    for s in ("2", "4"):
        d = rec[s]["direct"]
        assert "tpgsr_charbonnier_loss_fwd" in d and "tpgsr_charbonnier_loss_bwd" in d and "tpgsr_image_loss_finalize" in d
        assert "tpgsr_image_loss_fwd" not in d and "tpgsr_l1_loss_fwd" not in d and "tpgsr_image_loss_bwd" not in d
        assert d.count("tpgsr_copy_strided") == 2          # channels=3: the RGB prefixes of LR and HR


def test_engine_scale_is_the_modules_factor(rec):
    assert rec["2"]["scale"] == 2 and rec["4"]["scale"] == 4
    assert rec["srres_scale"] == 2 and rec["class_scale"] == 2
    for s in ("2", "4"):      # the HR grid is checked against the engine's factor
        e = rec[s]["wrong_hr"]
        assert e and e[0] == "ValueError" and f"{s}H, {s}W" in e[1]


def test_evaluator_pass_takes_both_factors(rec):
    for s in (2, 4):
        r = rec[f"eval_{s}"]
        assert r["sr"] == [6, 3, 16 * s, 64 * s] and r["priors"] == 0
        # one recorded forward plan behind the channel-prefix copy: no text-prior launch next to it
        assert r["direct"] == ["tpgsr_copy_strided", "tpgsr_copy", "tpgsr_copy"]
        assert "tpgsr_dilate2d" not in r["plan"] and r["plan"].count("tpgsr_tconv4s2_expand") == s // 2


def test_functional_op_fallback_and_refusals(rec):
    d = rec["dilated_8x8"]
    assert d["y"] == [2, 6, 10, 8] and "tpgsr_dilate2d" in d["direct"] and "tpgsr_tconv4s2_expand" not in d["direct"]
    assert rec["bad_form"] and rec["bad_form"][0] == "ValueError" and "no subpixel route" in rec["bad_form"][1]
    assert rec["bad_weight"] and rec["bad_weight"][0] == "ValueError"
    assert rec["cin5"] and rec["cin5"][0] == "ValueError" and "5 -> 3" in rec["cin5"][1]


@pytest.mark.parametrize("scale", [2, 4])
def test_fixtures_load_and_are_finite(scale):
    from make_golden_lapsrn import N_STORE
    from tpgsr_amd.model import lapsrn
    g = np.load(os.path.join(GOLD, f"lapsrn_x{scale}.npz"), allow_pickle=False)
    t = np.load(os.path.join(GOLD, f"train_lapsrn_x{scale}.npz"), allow_pickle=False)
    for path in (f"lapsrn_x{scale}.npz", f"train_lapsrn_x{scale}.npz"):
        assert os.path.getsize(os.path.join(GOLD, path)) < 700 * 1024
    assert g["y"].shape == t["sr_step0"].shape == (N_STORE[scale], 3, 16 * scale, 64 * scale)
    assert g["y_small"].shape == (2, 3, 12 * scale, 40 * scale)
    assert t["loss"].shape == (2,) and t["gnorm"].shape == (2,) and (t["loss"] > 0).all() and (t["gnorm"] > 0).all()
    for k in ("y", "y_small", "grad_norms", "grad_heads"):
        assert np.isfinite(g[k]).all() and g[k].size, k
    names = [n for n, _ in lapsrn.LapSRN(scale_factor=scale).named_parameters()]
    assert [str(n) for n in g["grad_names"]] == names
    live = np.array([scale == 4 or not n.startswith(("convt_I2", "convt_R2", "convt_F2")) for n in names])
    assert (g["grad_norms"][live] > 0).all() and (g["grad_norms"][~live] == 0).all()      # x2: the second stage has no gradient
    assert len(g["eval_sr"]) == len(g["eval_lr"]) == len(g["eval_hr"]) == 6
