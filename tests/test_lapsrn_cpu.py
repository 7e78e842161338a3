"""CPU: `--arch lapsrn` (LapSRN x2 / x4, L1_Charbonnier_loss) through the host layers -- constructor, state_dict layout against the
reference's (tests/golden/lapsrn_layouts.json), initialisation, refusals, the C ABI of the new entry points, and plan recording in dry-run
mode (TPGSR_PLAN_DRYRUN=1, the pattern of tests/test_plain_baselines_cpu.py) through `SRTrainStep` with the new criterion value and through
the prior-free evaluator pass; the committed fixtures."""
import json
import os
import sys

import pytest
import torch

from plain_arch_record import GOLD, ROOT, check_criterion_kernels, check_entry_points, check_evaluator_case, check_fixtures, record

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
    check_entry_points(NEW_SYMBOLS, None, 13)      # (the kernels went into source files the build already listed)


def test_form_table_of_the_transposed_convolution():
    from tpgsr_amd import functional as Fh
    assert Fh.tconv_k4s2_form(64, 64) == "subpixel"
    assert Fh.tconv_k4s2_form(3, 3) == Fh.tconv_k4s2_form(4, 4) == Fh.tconv_k4s2_form(2, 3) == "direct"
    assert Fh.tconv_k4s2_form(8, 8) == Fh.tconv_k4s2_form(5, 3) == "dilated"


IMPORTS = "from tpgsr_amd.model import lapsrn, srresnet"
CASES = r'''
for s in (2, 4):
    out[str(s)] = train_case(lambda: lapsrn.LapSRN(scale_factor=s), s, "l1_charbonnier")
    out[str(s)]["n_live"] = len([n for n, p in lapsrn.LapSRN(scale_factor=s).named_parameters()
                                 if s == 4 or not n.startswith(("convt_I2", "convt_R2", "convt_F2"))])
    out["eval_%d" % s] = eval_case(lambda: lapsrn.LapSRN(scale_factor=s), s)
out["srres_scale"] = srresnet.SRResNet()._engine().scale
out["class_scale"] = PlainSREngine.scale
'''
EXTRA = r'''
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
'''


@pytest.fixture(scope="module")
def rec():
    return record(IMPORTS, CASES, EXTRA)


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
    check_criterion_kernels(rec, ("2", "4"), "l1_charbonnier")


def test_engine_scale_is_the_modules_factor(rec):
    assert rec["2"]["scale"] == 2 and rec["4"]["scale"] == 4
    assert rec["srres_scale"] == 2 and rec["class_scale"] == 2
    for s in ("2", "4"):      # the HR grid is checked against the engine's factor
        e = rec[s]["wrong_hr"]
        assert e and e[0] == "ValueError" and f"{s}H, {s}W" in e[1]


def test_evaluator_pass_takes_both_factors(rec):
    for s in (2, 4):
        r = rec[f"eval_{s}"]
        check_evaluator_case(r, s)
        assert "tpgsr_dilate2d" not in r["plan"] and r["plan"].count("tpgsr_tconv4s2_expand") == s // 2


def test_functional_op_fallback_and_refusals(rec):
    d = rec["dilated_8x8"]
    assert d["y"] == [2, 6, 10, 8] and "tpgsr_dilate2d" in d["direct"] and "tpgsr_tconv4s2_expand" not in d["direct"]
    assert rec["bad_form"] and rec["bad_form"][0] == "ValueError" and "no subpixel route" in rec["bad_form"][1]
    assert rec["bad_weight"] and rec["bad_weight"][0] == "ValueError"
    assert rec["cin5"] and rec["cin5"][0] == "ValueError" and "5 -> 3" in rec["cin5"][1]


@pytest.mark.parametrize("scale", [2, 4])
def test_fixtures_load_and_are_finite(scale):
    import plain_arch_common as P
    check_fixtures(P.LAPSRN, scale)
