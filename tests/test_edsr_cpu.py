"""CPU: `--arch edsr` (EDSR x2 / x4) through the host layers -- constructor, state_dict layout against the reference's
(tests/golden/edsr_layouts.json), the reference constructor's initialisation (MeanShift included), parameter counts, refusals, FusedAdam
and frozen parameters, the C ABI of the new entry points, and plan recording in dry-run mode (TPGSR_PLAN_DRYRUN=1, the pattern of
tests/test_rrdb_cpu.py) through `SRTrainStep` with image_crit="l1" in both forms of the residual block and of conv_output and through the
prior-free evaluator pass; the committed fixtures."""
import inspect
import json
import os
import re
import sys

import pytest
import torch

from plain_arch_record import GOLD, ROOT, check_criterion_kernels, check_entry_points, check_evaluator_case, check_fixtures, record

sys.path.insert(0, ROOT)
sys.path.insert(0, GOLD)

NEW_SYMBOLS = ("tpgsr_conv3x3_narrow_fwd", "tpgsr_conv3x3_narrow_bwd_data", "tpgsr_conv3x3_narrow_bwd_weight")
FROZEN = ["sub_mean.weight", "sub_mean.bias", "add_mean.weight", "add_mean.bias"]


def test_constructor_signatures():
    from tpgsr_amd.model import edsr

    def sig(f):
        return [(p.name, p.default, p.kind) for p in list(inspect.signature(f).parameters.values())[1:]]

    POS, KW = inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.KEYWORD_ONLY
    assert sig(edsr.EDSR.__init__) == [("scale_factor", 2, POS), ("n_resblocks", 32, KW)]
    assert sig(edsr.MeanShift.__init__) == [("rgb_mean", inspect.Parameter.empty, POS), ("sign", inspect.Parameter.empty, POS)]
    assert sig(edsr._Residual_Block.__init__) == []
    assert "NOT the reference's" in edsr.EDSR.__doc__ and "what the reference's constructor does" in edsr.__doc__


@pytest.mark.parametrize("nb", [2, 32])
@pytest.mark.parametrize("scale", [2, 4])
def test_state_dict_layout_equals_the_reference(scale, nb):
    from make_golden_next import generic_recipe
    from tpgsr_amd.model import edsr
    layouts = json.load(open(os.path.join(GOLD, "edsr_layouts.json")))
    lay = layouts[f"x{scale}_nb{nb}"]
    net = edsr.EDSR(scale_factor=scale, n_resblocks=nb)
    assert [(k, list(v.shape)) for k, v in net.state_dict().items()] == [(a, b) for a, b in lay]
    assert [k for k, p in net.named_parameters() if not p.requires_grad] == layouts[f"x{scale}_nb{nb}_frozen"] == FROZEN
    keys = [k for k, _ in lay]
    assert keys[:3] == ["sub_mean.weight", "sub_mean.bias", "conv_input.weight"] and keys[-3:] == ["conv_output.weight", "add_mean.weight", "add_mean.bias"]
    assert ("upscale.2.weight" in keys) == (scale == 4) and "upscale.0.weight" in keys and "upscale.1.weight" not in keys
    assert sum(k.startswith("residual.") for k in keys) == 2 * nb and not any(k.endswith(".bias") for k in keys if "mean" not in k)
    if nb == 32:
        assert len(keys) == {2: 72, 4: 73}[scale]
    ckpt = generic_recipe({k: torch.empty(s) for k, s in lay}, 7)               # a checkpoint in the reference's layout loads strictly
    res = net.load_state_dict(ckpt, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in net.state_dict().items():
        assert torch.equal(v, ckpt[k]), k
    assert [k for k, p in net.named_parameters() if not p.requires_grad] == FROZEN      # loading does not thaw them


def test_parameter_counts():
    from tpgsr_amd.model import edsr
    for s, want in ((2, 40711704), (4, 43071000)):
        net = edsr.EDSR(scale_factor=s)
        assert sum(p.numel() for p in net.parameters()) == want
        assert sum(p.numel() for p in net.parameters() if not p.requires_grad) == 24


def test_initialisation_is_the_reference_constructors():
    """every convolution weight N(0, sqrt(2 / (k^2 Cout))), the two MeanShift layers included: NOT the identity, biases zero, frozen"""
    from tpgsr_amd.model import edsr
    torch.manual_seed(5)
    net = edsr.EDSR(scale_factor=4, n_resblocks=2)
    for name, p in net.named_parameters():
        if name.endswith(".bias"):
            assert name in FROZEN and float(p.abs().max()) == 0.0 and not p.requires_grad
            continue
        cout, _, kh, kw = p.shape
        std = (2.0 / (kh * kw * cout)) ** 0.5
        v = p.detach().double()
        assert float(v.abs().max()) <= 6.5 * std, name                      # (4.7 M draws at most: 6.5 sigma is 1e-10 per draw)
        if p.numel() >= 4096:
            se = std / (2 * p.numel()) ** 0.5                               # standard error of a sample's standard deviation
            assert abs(float(v.std()) - std) < 6 * se and abs(float(v.mean())) < 6 * std / p.numel() ** 0.5, name
        assert p.requires_grad == (name not in FROZEN)
    # the MeanShift weights over many constructions: the spread of N(0, sqrt(2/3)), never the identity
    draws = []
    for _ in range(60):
        n2 = edsr.EDSR(scale_factor=2, n_resblocks=0)
        for m in (n2.sub_mean, n2.add_mean):
            assert not torch.equal(m.weight.detach().view(3, 3), torch.eye(3)) and float(m.bias.abs().max()) == 0.0
            assert not m.weight.requires_grad and not m.bias.requires_grad
            draws.append(m.weight.detach().reshape(-1))
    d = torch.cat(draws).double()                                           # 1080 draws
    std = (2.0 / 3.0) ** 0.5
    assert abs(float(d.std()) - std) < 6 * std / (2 * d.numel()) ** 0.5 and abs(float(d.mean())) < 6 * std / d.numel() ** 0.5
    # standing alone, MeanShift is what the reference's class builds
    ms = edsr.MeanShift((0.4488, 0.4371, 0.4040), -1)
    assert torch.equal(ms.weight.view(3, 3), torch.eye(3)) and torch.equal(ms.bias, -torch.tensor([0.4488, 0.4371, 0.4040]))


def test_refusals():
    from tpgsr_amd import functional as Fh
    from tpgsr_amd.model import edsr
    for s in (1, 3, 8):
        with pytest.raises(ValueError, match="scale_factor"):
            edsr.EDSR(scale_factor=s, n_resblocks=1)
    with pytest.raises(TypeError):
        edsr.EDSR(2, 1)                                                     # n_resblocks is keyword only
    net = edsr.EDSR(n_resblocks=1)
    with pytest.raises(ValueError, match="form"):
        net.set_form("inplace")
    with pytest.raises(ValueError, match="form"):
        net.set_tail_form("direct")
    x = torch.zeros(1, 5, 7, 8)
    w = torch.zeros(8, 8, 3, 3)
    with pytest.raises(ValueError, match="form"):
        Fh.res_block(x, w, w, form="in-place")
    with pytest.raises(ValueError, match="channels"):
        Fh.res_block(x, torch.zeros(12, 12, 3, 3), w)
    with pytest.raises(ValueError, match="channels"):
        Fh.res_block(x, w, torch.zeros(8, 12, 3, 3))
    with pytest.raises(ValueError, match="3x3"):
        Fh.res_block(x, torch.zeros(8, 8, 1, 1), w)
    with pytest.raises(ValueError, match="multiple of 4"):
        Fh.res_block(torch.zeros(1, 5, 7, 6), torch.zeros(6, 6, 3, 3), torch.zeros(6, 6, 3, 3), form="fused")
    with pytest.raises(ValueError, match="not \\(N, H, W, C\\)"):
        Fh.res_block(torch.zeros(5, 7, 8), w, w)
    with pytest.raises(ValueError, match="form"):
        Fh.conv2d_narrow(x, torch.zeros(3, 8, 3, 3), form="direct")
    with pytest.raises(ValueError, match="weight"):
        Fh.conv2d_narrow(x, torch.zeros(5, 8, 3, 3))
    with pytest.raises(ValueError, match="input"):
        Fh.conv2d_narrow(x, torch.zeros(3, 12, 3, 3))
    with pytest.raises(ValueError, match="multiple of 4"):
        Fh.conv2d_narrow(torch.zeros(1, 5, 7, 6), torch.zeros(3, 6, 3, 3), form="narrow")
    with pytest.raises(RuntimeError, match="no CPU|GPU only"):
        Fh.res_block(x, w, w)
    with pytest.raises(RuntimeError, match="no CPU|GPU only"):
        Fh.conv2d_narrow(x, torch.zeros(3, 8, 3, 3), form="narrow")
    with pytest.raises(RuntimeError, match="no CPU|GPU only"):
        net(torch.zeros(1, 3, 16, 64))
    with pytest.raises(ValueError, match="EDSR: input"):
        net(torch.zeros(1, 4, 16, 64))
    assert Fh.RES_FORMS == ("fused", "composed") and Fh.RES_DEFAULT_FORM in Fh.RES_FORMS
    assert Fh.NARROW_FORMS == ("narrow", "matrix") and Fh.NARROW_DEFAULT_FORM in Fh.NARROW_FORMS


def test_new_entry_points_are_declared_bound_and_registered():
    check_entry_points(NEW_SYMBOLS, "conv_narrow.hip", 13)
    # the host-side mirror of the kernels' constants
    from tpgsr_amd import kernels as K
    src = open(os.path.join(ROOT, "tpgsr_amd", "csrc", "conv_narrow.hip")).read()
    for name, value in (("kRun", K.NARROW_RUN), ("kWaves", K.NARROW_WAVES), ("kGridCap", K.NARROW_GRID_CAP), ("kMaxCin", K.NARROW_MAX_CIN),
                        ("kMaxCout", K.NARROW_MAX_COUT)):
        assert re.search(r"constexpr int %s = %d;" % (name, value), src), name


def test_fused_adam_accepts_declared_frozen_parameters_only():
    from tpgsr_amd.model import edsr, srresnet
    from tpgsr_amd.optim import FusedAdam
    net = edsr.EDSR(n_resblocks=1)
    assert list(edsr.EDSR.FROZEN_BY_ENGINE) == FROZEN
    FusedAdam([net], clip_modules=[net])
    # a further parameter frozen by hand is not covered by the declaration
    net.conv_mid.weight.requires_grad = False
    with pytest.raises(NotImplementedError, match="conv_mid.weight"):
        FusedAdam([net])
    # a module that declares nothing is refused as before
    other = srresnet.SRResNet(scale_factor=2)
    name, p = next(iter(other.named_parameters()))
    p.requires_grad = False
    assert not hasattr(type(other), "FROZEN_BY_ENGINE")
    with pytest.raises(NotImplementedError, match="frozen parameters"):
        FusedAdam([other])


IMPORTS = "from tpgsr_amd.model import edsr"
CASES = r'''
def edsr_net(s, form, tail=None):
    net = edsr.EDSR(scale_factor=s, n_resblocks=NB)
    net.set_form(form)
    net.set_tail_form(tail)
    return net

out.update(res_default=Fh.RES_DEFAULT_FORM, tail_default=Fh.NARROW_DEFAULT_FORM)
for form, tail in (("fused", "narrow"), ("composed", "matrix"), (None, None)):
    for s in (2, 4):
        out[str(form) + str(s)] = train_case(lambda: edsr_net(s, form, tail), s, "l1")
for s in (2, 4):
    for form in Fh.RES_FORMS:
        out["eval_%s_%d" % (form, s)] = eval_case(lambda: edsr_net(s, form), s)
'''
EXTRA = r'''
# a channel count that is no multiple of 4: form=None falls back to the composed form
del direct[:]
x = torch.rand(1, 5, 8, 6).requires_grad_(True)
w1, w2 = [torch.rand(6, 6, 3, 3).requires_grad_(True) for _ in range(2)]
y = Fh.res_block(x, w1, w2)
y.sum().backward()
out["odd"] = dict(direct=list(direct), y=list(y.shape))
# the world-size refusal of the operator-level backbones
out["world"] = err(lambda: SRTrainStep(edsr.EDSR(n_resblocks=1).train(), image_crit="l1", channels=3, world_size=2))
'''


@pytest.fixture(scope="module")
def rec():
    return record(IMPORTS, CASES, EXTRA)


NB = 2
ELEMENTWISE = ("tpgsr_scaled_add", "tpgsr_add", "tpgsr_add_n", "tpgsr_act_bwd", "tpgsr_affine_act", "tpgsr_copy", "tpgsr_copy_strided")


@pytest.mark.timeout(600)
@pytest.mark.parametrize("scale", [2, 4])
def test_fused_plan_of_the_train_step(rec, scale):
    r = rec[f"fused{scale}"]
    n_up = 1 if scale == 2 else 2
    n_mat = 2 * NB + 4 + n_up       # on the convolution launches: sub_mean, conv_input, the blocks, conv_mid, the up-sampling stages, add_mean
    assert r["key"] == ["(4, 3, 16, 64)", "True", "0", "x3"]
    assert r["sr"] == [4, 3, 16 * scale, 64 * scale] and r["pooled"] and not r["has_prior"] and r["scale"] == scale
    fwd, bwd = r["fwd"], r["bwd"]
    assert fwd.count("tpgsr_conv_fwd") == n_mat and fwd.count("tpgsr_conv3x3_narrow_fwd") == 1
    # one element-wise launch per block forward, no ReLU launch, no pixel-shuffle launch; the long skip is the one tpgsr_add
    assert fwd.count("tpgsr_scaled_add") == NB and fwd.count("tpgsr_add") == 1 and "tpgsr_affine_act" not in fwd
    assert sum(fwd.count(k) for k in ELEMENTWISE) == NB + 1
    assert "join" not in fwd
    # backward: res_scale * dy and dx = dy + T per block -- two element-wise launches -- and the long skip's gradient sum; no ReLU backward
    assert bwd.count("tpgsr_scaled_add") == NB and bwd.count("tpgsr_add") == NB + 1 and "tpgsr_act_bwd" not in bwd
    assert sum(bwd.count(k) for k in ELEMENTWISE) == 2 * NB + 1
    # weight gradients: none for the two frozen layers; data gradients: none for sub_mean / conv_input (the image needs no gradient)
    assert bwd.count("tpgsr_conv_wgrad") == n_mat - 2 and bwd.count("tpgsr_conv_fwd") == n_mat - 2
    assert bwd.count("tpgsr_conv3x3_narrow_bwd_data") == 1 and bwd.count("tpgsr_conv3x3_narrow_bwd_weight") == 1
    assert bwd.count("tpgsr_reduce_partials") == 1                      # conv_output's partial sums, into the sink
    assert bwd.count("tpgsr_wgrad_reduce_program") == 1 and "tpgsr_wgrad_reduce" not in bwd
    assert "fork" in bwd and bwd[-1] == "join"
    e = r["wrong_hr"]
    assert e and e[0] == "ValueError" and f"{scale}H, {scale}W" in e[1]


@pytest.mark.parametrize("scale", [2, 4])
def test_composed_plan_and_matrix_tail(rec, scale):
    r, f = rec[f"composed{scale}"], rec[f"fused{scale}"]
    fwd, bwd = r["fwd"], r["bwd"]
    assert "tpgsr_conv3x3_narrow_fwd" not in fwd and "tpgsr_conv3x3_narrow_bwd_data" not in bwd and "tpgsr_reduce_partials" not in bwd
    assert fwd.count("tpgsr_conv_fwd") == f["fwd"].count("tpgsr_conv_fwd") + 1
    assert fwd.count("tpgsr_affine_act") == NB and bwd.count("tpgsr_act_bwd") == NB          # the ReLU pass and its backward
    assert fwd.count("tpgsr_scaled_add") == NB and bwd.count("tpgsr_scaled_add") == NB
    assert bwd.count("tpgsr_add") == NB + 1                                                   # the blocks' forks and the long skip
    assert r["sr"] == [4, 3, 16 * scale, 64 * scale] and r["scale"] == scale


@pytest.mark.parametrize("scale", [2, 4])
def test_default_plan_is_the_default_forms(rec, scale):
    r = rec[f"None{scale}"]
    same = rec[("fused" if rec["res_default"] == "fused" else "composed") + str(scale)]
    assert r["fwd"].count("tpgsr_scaled_add") == same["fwd"].count("tpgsr_scaled_add")
    assert r["fwd"].count("tpgsr_affine_act") == (0 if rec["res_default"] == "fused" else NB)
    assert r["fwd"].count("tpgsr_conv3x3_narrow_fwd") == (1 if rec["tail_default"] == "narrow" else 0)


def test_l1_criterion_records_its_kernels(rec):
    check_criterion_kernels(rec, ("fused2", "fused4", "composed2"), "l1")


def test_evaluator_pass_takes_both_factors(rec):
    for s in (2, 4):
        for form in ("fused", "composed"):
            r = rec[f"eval_{form}_{s}"]
            check_evaluator_case(r, s)
            assert r["plan"].count("tpgsr_scaled_add") == NB and r["plan"].count("tpgsr_conv3x3_narrow_fwd") == 1
            assert r["plan"].count("tpgsr_affine_act") == (0 if form == "fused" else NB)      # ReLU in conv1's epilogue / a pass of its own


def test_odd_channel_counts_take_the_composed_form(rec):
    d = rec["odd"]
    assert d["y"] == [1, 5, 8, 6] and d["direct"].count("tpgsr_affine_act") == 1 and d["direct"].count("tpgsr_act_bwd") == 1


def test_gradient_exchange_stays_refused(rec):
    e = rec["world"]
    assert e is not None and e[0] == "NotImplementedError" and "gradient exchange" in e[1], e


@pytest.mark.parametrize("scale", [2, 4])
def test_fixtures_load_and_are_finite(scale):
    import plain_arch_common as P
    from make_golden_edsr import FROZEN as GEN_FROZEN
    assert list(GEN_FROZEN) == FROZEN
    check_fixtures(P.EDSR, scale)
