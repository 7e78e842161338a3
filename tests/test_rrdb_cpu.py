"""CPU: `--arch esrgan` (RRDBNet x2 / x4) through the host layers -- constructor, state_dict layout against the reference's
(tests/golden/rrdb_layouts.json), initialisation, refusals, the C ABI of the new entry points, and plan recording in dry-run mode
(TPGSR_PLAN_DRYRUN=1, the pattern of tests/test_lapsrn_cpu.py) through `SRTrainStep` with image_crit="l1" in both forms of the dense
block and through the prior-free evaluator pass; the committed fixtures."""
import inspect
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

NEW_SYMBOLS = ("tpgsr_leaky_relu_window", "tpgsr_scaled_add", "tpgsr_dense_bwd_step")


def test_constructor_signatures():
    from tpgsr_amd.model import esrgan

    def sig(f):
        return [(p.name, p.default) for p in list(inspect.signature(f).parameters.values())[1:]]

    assert sig(esrgan.RRDBNet.__init__) == [("scale_factor", 2), ("in_nc", 3), ("out_nc", 3), ("nf", 64), ("nb", 23), ("gc", 32)]
    assert sig(esrgan.ResidualDenseBlock_5C.__init__) == [("nf", 64), ("gc", 32), ("bias", True)]
    assert sig(esrgan.RRDB.__init__) == [("nf", inspect.Parameter.empty), ("gc", 32)]
    assert not hasattr(esrgan, "SubDiscriminator") and not hasattr(esrgan, "conv_block")      # dead code in the reference: not built


@pytest.mark.parametrize("nb", [2, 23])
@pytest.mark.parametrize("scale", [2, 4])
def test_state_dict_layout_equals_the_reference(scale, nb):
    from make_golden_next import generic_recipe
    from tpgsr_amd.model import esrgan
    lay = json.load(open(os.path.join(GOLD, "rrdb_layouts.json")))[f"x{scale}_nb{nb}"]
    net = esrgan.RRDBNet(scale_factor=scale, nb=nb)
    assert [(k, list(v.shape)) for k, v in net.state_dict().items()] == [(a, b) for a, b in lay]
    keys = [k for k, _ in lay]
    assert keys[:2] == ["conv_first.weight", "conv_first.bias"] and keys[-2:] == ["conv_last.weight", "conv_last.bias"]
    assert ("upconv2.weight" in keys) == (scale == 4) and "upconv1.weight" in keys and "upconv3.weight" not in keys
    assert sum(k.startswith("RRDB_trunk.") for k in keys) == nb * 3 * 5 * 2      # every convolution with bias
    ckpt = generic_recipe({k: torch.empty(s) for k, s in lay}, 7)               # a checkpoint in the reference's layout loads strictly
    res = net.load_state_dict(ckpt, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in net.state_dict().items():
        assert torch.equal(v, ckpt[k]), k


def test_initialisation_is_pytorchs_default():
    """nn.Conv2d's default: kaiming_uniform(a = sqrt(5)) = U(+-1 / sqrt(fan_in)) for weight and bias alike; the reference applies none of its own"""
    from tpgsr_amd.model import esrgan
    torch.manual_seed(3)
    net = esrgan.RRDBNet(scale_factor=4, nb=2)
    for name, p in net.named_parameters():
        mod = net.get_submodule(name.rsplit(".", 1)[0])
        bound = float(torch.tensor(1.0 / (mod.in_channels * 9) ** 0.5, dtype=torch.float32))      # (the sampler's float32 bound)
        assert float(p.detach().abs().max()) <= bound, name
        if p.numel() >= 4096:      # ... and fills the interval: a uniform sample's spread
            assert float(p.detach().abs().max()) > 0.98 * bound and abs(float(p.detach().std()) - bound / 3 ** 0.5) < 0.05 * bound, name


def test_refusals():
    from tpgsr_amd import functional as Fh
    from tpgsr_amd.model import esrgan
    for s in (1, 3, 8):
        with pytest.raises(ValueError, match="scale_factor"):
            esrgan.RRDBNet(scale_factor=s, nb=1)
    net = esrgan.RRDBNet(nb=1)
    with pytest.raises(ValueError, match="form"):
        net.set_form("fused")
    x = torch.zeros(1, 5, 7, 64)
    ws = [torch.zeros(32 if k < 4 else 64, 64 + 32 * k, 3, 3) for k in range(5)]
    with pytest.raises(ValueError, match="form"):
        Fh.dense_block(x, ws, None, form="in-place")
    with pytest.raises(ValueError, match="five"):
        Fh.dense_block(x, ws[:4], None)
    with pytest.raises(ValueError, match="multiples of 4"):
        Fh.dense_block(torch.zeros(1, 5, 7, 6), [torch.zeros(2 if k < 4 else 6, 6 + 2 * k, 3, 3) for k in range(5)], None, form="inplace")
    with pytest.raises(RuntimeError, match="no CPU|GPU only"):
        Fh.dense_block(x, ws, None)
    with pytest.raises(RuntimeError, match="no CPU|GPU only"):
        Fh.scaled_add(x, x, 0.2)
    with pytest.raises(RuntimeError, match="no CPU|GPU only"):
        net(torch.zeros(1, 3, 16, 64))
    with pytest.raises(ValueError, match="RRDBNet: input"):
        net(torch.zeros(1, 4, 16, 64))


def test_new_entry_points_are_declared_bound_and_registered():
    from tpgsr_amd import _lib
    from tpgsr_amd.build import SOURCES
    header = open(os.path.join(ROOT, "include", "tpgsr_hip.h")).read()
    plan = open(os.path.join(ROOT, "tpgsr_amd", "csrc", "plan.cpp")).read()
    assert "dense.hip" in SOURCES
    for sym in NEW_SYMBOLS:
        assert sym in _lib.EXPORTED_SYMBOLS
        assert re.search(r"\bint\s+%s\s*\(" % sym, header)
        assert "TPGSR_REG(%s)" % sym in plan
        fn = getattr(_lib.load(), sym)
        assert len(fn.argtypes) <= 24 + 1
    assert len(_lib.ABI_STRUCTS) == 13      # scalar and pointer parameters only: no new argument block


RECORD = r'''
import json, sys, torch
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
from tpgsr_amd import kernels as K
assert K.DRYRUN
from tpgsr_amd import functional as Fh
from tpgsr_amd.engine_functional import PlainSREngine
from tpgsr_amd.interfaces.super_resolution import SRTrainStep, TextSREvaluator
from tpgsr_amd.model import esrgan
from tpgsr_amd.model.crnn import crnn
from plan_signature import signature

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

NB = 2
out = {"default_form": Fh.DENSE_DEFAULT_FORM}
torch.manual_seed(0)
for form in ("inplace", "composed"):
    for s in (2, 4):
        del direct[:]
        net = esrgan.RRDBNet(scale_factor=s, nb=NB).train()
        net.set_form(form)
        ts = SRTrainStep(net, precision="x3", image_crit="l1", channels=3)
        loss = ts.step(torch.rand(4, 4, 16, 64), torch.rand(4, 4, 16 * s, 64 * s))
        eng = net._engine()
        assert isinstance(eng, PlainSREngine) and eng.record and tuple(loss.shape) == ()
        (key, pl), = eng._plans.items()
        lines = signature(eng._plans)                 # runs every plan: the native executor checks entry point and argument count of every op
        a, b = ts.pool.ranges[id(net)]
        out[form + str(s)] = dict(key=[str(k) for k in key], fwd=[o[0] for o in pl["fwd"].ops], bwd=[o[0] for o in pl["bwd"].ops],
                                  direct=list(direct), sr=list(ts.last_sr.shape), scale=eng.scale, nsig=len(lines),
                                  pooled=bool(eng.arena.external is not None and b - a == eng.arena.numel),
                                  sunk=all(p.grad is not None for p in net.parameters()), has_prior=("prior" in pl or "dprior" in pl),
                                  wrong_hr=err(lambda: ts.step(torch.rand(4, 4, 16, 64), torch.rand(4, 4, 8 * s, 32 * s))))

rec = crnn.CRNN(32, 1, 37, 256).eval()
for s in (2, 4):
    del direct[:]
    net = esrgan.RRDBNet(scale_factor=s, nb=NB).eval()
    ev = TextSREvaluator([net], None, recognizer=rec, channels=3)
    srs, priors = ev.super_resolve(torch.rand(6, 4, 16, 64))
    (pl,) = net._engine()._plans.values()
    out["eval_%%d" %% s] = dict(direct=list(direct), sr=list(srs[0].shape), priors=len(priors), plan=[o[0] for o in pl["fwd"].ops])

# odd channel counts: form=None falls back to the composed form
del direct[:]
x = torch.rand(1, 5, 7, 6).requires_grad_(True)
ws = [torch.rand(2 if k < 4 else 6, 6 + 2 * k, 3, 3).requires_grad_(True) for k in range(5)]
y = Fh.dense_block(x, ws, None)
y.sum().backward()
out["odd"] = dict(direct=list(direct), y=list(y.shape))
print("RESULT " + json.dumps(out))
'''


@pytest.fixture(scope="module")
def rec():
    env = dict(os.environ, TPGSR_PLAN_DRYRUN="1")
    for k in [k for k in env if k.startswith("TPGSR_") and k != "TPGSR_PLAN_DRYRUN"]:
        del env[k]
    r = subprocess.run([sys.executable, "-c", RECORD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"))], capture_output=True, text=True,
                       env=env, timeout=550)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


NB = 2


@pytest.mark.timeout(600)
@pytest.mark.parametrize("scale", [2, 4])
def test_in_place_plan_of_the_train_step(rec, scale):
    r = rec[f"inplace{scale}"]
    n_up = 1 if scale == 2 else 2
    n_conv = 15 * NB + 4 + n_up
    assert r["key"] == ["(4, 3, 16, 64)", "True", "0", "x3"]
    assert r["sr"] == [4, 3, 16 * scale, 64 * scale] and r["pooled"] and r["sunk"] and not r["has_prior"] and r["scale"] == scale
    fwd, bwd = r["fwd"], r["bwd"]
    assert fwd.count("tpgsr_conv_fwd") == n_conv
    assert fwd.count("tpgsr_leaky_relu_window") == 4 * 3 * NB       # one per growing convolution
    assert fwd.count("tpgsr_scaled_add") == 4 * NB                  # three blocks and the RRDB's own residual
    assert fwd.count("tpgsr_copy_strided") == 3 * NB                # x into the buffer, once per dense block: no concatenation is copied
    assert fwd.count("tpgsr_add") == 1                              # fea + trunk
    i_add = fwd.index("tpgsr_add")
    assert "tpgsr_scaled_add" not in fwd[i_add:] and "tpgsr_leaky_relu_window" not in fwd[i_add:]      # ... behind the trunk
    assert fwd.count("tpgsr_leaky_relu_fwd") == n_up + 1 and fwd.count("tpgsr_resize_nearest_fwd") == n_up
    assert "join" not in fwd
    # backward: five passes of the in-place step per block (four masks, the last writes dx), res_scale * dy by scaled_add (one per block
    # and one per RRDB); no slice copy, no LeakyReLU backward inside the trunk; one gradient sum per fork (the RRDBs' and the long skip)
    assert bwd.count("tpgsr_dense_bwd_step") == 5 * 3 * NB and bwd.count("tpgsr_scaled_add") == 4 * NB
    assert "tpgsr_copy_strided" not in bwd and bwd.count("tpgsr_leaky_relu_bwd") == n_up + 1
    assert bwd.count("tpgsr_add") == NB + 1
    assert bwd.count("tpgsr_conv_wgrad") == n_conv and bwd.count("tpgsr_conv_fwd") == n_conv - 1      # (conv_first has no data gradient)
    assert bwd.count("tpgsr_wgrad_reduce_program") == 1 and "tpgsr_wgrad_reduce" not in bwd
    assert "fork" in bwd and bwd[-1] == "join"
    e = r["wrong_hr"]
    assert e and e[0] == "ValueError" and f"{scale}H, {scale}W" in e[1]


@pytest.mark.parametrize("scale", [2, 4])
def test_composed_plan_holds_no_window_kernel(rec, scale):
    r = rec[f"composed{scale}"]
    fwd, bwd = r["fwd"], r["bwd"]
    assert "tpgsr_leaky_relu_window" not in fwd and "tpgsr_dense_bwd_step" not in bwd
    assert fwd.count("tpgsr_copy_strided") == 2 * 4 * 3 * NB       # two slice copies per concatenation
    assert fwd.count("tpgsr_scaled_add") == 4 * NB and fwd.count("tpgsr_conv_fwd") == rec[f"inplace{scale}"]["fwd"].count("tpgsr_conv_fwd")
    assert r["sr"] == [4, 3, 16 * scale, 64 * scale] and r["sunk"] and r["scale"] == scale


def test_l1_criterion_records_its_kernels(rec):
    for k in ("inplace2", "inplace4", "composed2"):
        d = rec[k]["direct"]
        assert "tpgsr_l1_loss_fwd" in d and "tpgsr_l1_loss_bwd" in d
        assert "tpgsr_charbonnier_loss_fwd" not in d and "tpgsr_image_loss_fwd" not in d
        assert d.count("tpgsr_copy_strided") == 2          # channels=3: the RGB prefixes of LR and HR


def test_evaluator_pass_takes_both_factors(rec):
    for s in (2, 4):
        r = rec[f"eval_{s}"]
        assert r["sr"] == [6, 3, 16 * s, 64 * s] and r["priors"] == 0
        assert r["direct"] == ["tpgsr_copy_strided", "tpgsr_copy", "tpgsr_copy"]
        want = "tpgsr_leaky_relu_window" if rec["default_form"] == "inplace" else "tpgsr_leaky_relu_fwd"
        assert r["plan"].count(want) >= 4 * 3 * NB


def test_odd_channel_counts_take_the_composed_form(rec):
    d = rec["odd"]
    assert d["y"] == [1, 5, 7, 6] and "tpgsr_leaky_relu_window" not in d["direct"] and d["direct"].count("tpgsr_scaled_add") == 2


@pytest.mark.parametrize("scale", [2, 4])
def test_fixtures_load_and_are_finite(scale):
    from make_golden_rrdb import DEPTHS, N_SMALL, N_STORE
    from tpgsr_amd.model import esrgan
    for path in (f"rrdb_x{scale}.npz", f"train_rrdb_x{scale}.npz"):
        assert os.path.getsize(os.path.join(GOLD, path)) < 700 * 1000, path
    assert os.path.getsize(os.path.join(GOLD, "rrdb_layouts.json")) < 700 * 1000
    g = np.load(os.path.join(GOLD, f"rrdb_x{scale}.npz"), allow_pickle=False)
    t = np.load(os.path.join(GOLD, f"train_rrdb_x{scale}.npz"), allow_pickle=False)
    for nb in DEPTHS:
        pre = f"nb{nb}_"
        assert g[pre + "y"].shape == t[pre + "sr_step0"].shape == (N_STORE[scale], 3, 16 * scale, 64 * scale)
        assert g[pre + "y_small"].shape == (N_SMALL, 3, 12 * scale, 40 * scale)
        assert t[pre + "loss"].shape == (2,) and t[pre + "gnorm"].shape == (2,) and (t[pre + "loss"] > 0).all() and (t[pre + "gnorm"] > 0).all()
        for k in ("y", "y_small", "grad_norms", "grad_heads"):
            assert np.isfinite(g[pre + k]).all() and g[pre + k].size, k
        names = [n for n, _ in esrgan.RRDBNet(scale_factor=scale, nb=nb).named_parameters()]
        assert [str(n) for n in g[pre + "grad_names"]] == names
        assert (g[pre + "grad_norms"] > 0).all()
    assert len(g["eval_sr"]) == len(g["eval_lr"]) == len(g["eval_hr"]) == 6
