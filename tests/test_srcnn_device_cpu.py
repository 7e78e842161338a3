"""CPU: `--arch srcnn` (SRCNN x2 / x4) as a device backbone, through the host layers -- constructor, state_dict layout against the
reference's (tests/golden/srcnn_layouts.json), initial values against nn.Conv2d's under one seed, refusals, the C ABI of the new entry
points, and plan recording in dry-run mode (TPGSR_PLAN_DRYRUN=1, the pattern of tests/test_edsr_cpu.py) through `SRTrainStep` with
image_crit="mse" under both forms of conv3 and through the prior-free evaluator pass; the CPU input's ATen path against the float64
restatement; the committed fixtures.  (tests/test_srcnn_cpu.py keeps checking the CPU path against BASELINE config C1's fixture.)"""
import inspect
import json
import os
import re
import sys

import pytest
import torch

from plain_arch_record import GOLD, ROOT, check_entry_points, check_evaluator_case, check_fixtures, record

sys.path.insert(0, ROOT)
sys.path.insert(0, GOLD)

NEW_SYMBOLS = ("tpgsr_conv5x5_narrow_fwd", "tpgsr_conv5x5_narrow_bwd_data", "tpgsr_conv5x5_narrow_bwd_weight")
KEYS = ["conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "conv3.weight", "conv3.bias"]


def test_constructor_signature_and_class():
    from tpgsr_amd.model import srcnn
    from tpgsr_amd.model.nn_params import EngineHolder
    sig = [(p.name, p.default) for p in list(inspect.signature(srcnn.SRCNN.__init__).parameters.values())[1:]]
    assert sig == [("scale_factor", 2), ("in_planes", 3), ("STN", False), ("height", 32), ("width", 128)]
    assert issubclass(srcnn.SRCNN, EngineHolder) and "deliberate stock-PyTorch path" in srcnn.__doc__
    net = srcnn.SRCNN(scale_factor=4)
    assert net.upscale_factor == 4 and net.stn is False and net.tail_form is None


@pytest.mark.parametrize("scale", [2, 4])
def test_state_dict_layout_equals_the_reference(scale):
    from make_golden_next import generic_recipe
    from tpgsr_amd.model import srcnn
    lay = json.load(open(os.path.join(GOLD, "srcnn_layouts.json")))[f"x{scale}"]
    net = srcnn.SRCNN(scale_factor=scale)
    assert [(k, list(v.shape)) for k, v in net.state_dict().items()] == [(a, b) for a, b in lay]
    assert [k for k, _ in lay] == KEYS and sum(p.numel() for p in net.parameters()) == 20099
    assert all(p.requires_grad for p in net.parameters())
    ckpt = generic_recipe({k: torch.empty(s) for k, s in lay}, 7)               # a checkpoint in the reference's layout loads strictly
    res = net.load_state_dict(ckpt, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in net.state_dict().items():
        assert torch.equal(v, ckpt[k]), k


def test_initial_values_are_nn_conv2ds_under_one_seed():
    """the reference builds nn.Conv2d(3, 64, 9), nn.Conv2d(64, 32, 1), nn.Conv2d(32, 3, 5) in this order: the same draws, bit for bit"""
    from tpgsr_amd.model import srcnn
    torch.manual_seed(11)
    net = srcnn.SRCNN()
    torch.manual_seed(11)
    want = [torch.nn.Conv2d(3, 64, 9, padding=4), torch.nn.Conv2d(64, 32, 1), torch.nn.Conv2d(32, 3, 5, padding=2)]
    for ours, ref in zip((net.conv1, net.conv2, net.conv3), want):
        assert torch.equal(ours.weight, ref.weight) and torch.equal(ours.bias, ref.bias)
        assert ours.padding == ref.padding and ours.kernel_size == ref.kernel_size


def test_refusals():
    from tpgsr_amd import functional as Fh
    from tpgsr_amd.model import srcnn
    with pytest.raises(NotImplementedError, match="STN"):
        srcnn.SRCNN(STN=True)
    net = srcnn.SRCNN()
    with pytest.raises(ValueError, match="form"):
        net.set_tail_form("direct")
    for form in Fh.NARROW_FORMS + (None,):
        net.set_tail_form(form)
        assert net.tail_form == form
    x = torch.zeros(1, 5, 7, 8)
    w = torch.zeros(3, 8, 5, 5)
    with pytest.raises(ValueError, match="form"):
        Fh.conv2d_narrow5x5(x, w, form="direct")
    with pytest.raises(ValueError, match="weight"):
        Fh.conv2d_narrow5x5(x, torch.zeros(5, 8, 5, 5))
    with pytest.raises(ValueError, match="weight"):
        Fh.conv2d_narrow5x5(x, torch.zeros(3, 8, 3, 3))
    with pytest.raises(ValueError, match="input"):
        Fh.conv2d_narrow5x5(x, torch.zeros(3, 12, 5, 5))
    with pytest.raises(ValueError, match="bias"):
        Fh.conv2d_narrow5x5(x, w, torch.zeros(2))
    with pytest.raises(ValueError, match="multiple of 4"):
        Fh.conv2d_narrow5x5(torch.zeros(1, 5, 7, 6), torch.zeros(3, 6, 5, 5), form="narrow")
    with pytest.raises(ValueError, match="multiple of 4"):
        Fh.conv2d_narrow5x5(torch.zeros(1, 5, 7, 68), torch.zeros(3, 68, 5, 5), form="narrow")
    with pytest.raises(RuntimeError, match="no CPU|GPU only"):
        Fh.conv2d_narrow5x5(x, w, form="narrow")
    assert Fh.NARROW5_DEFAULT_FORM in Fh.NARROW_FORMS
    # conv2d_narrow keeps its contract: a 5x5 weight is refused there
    with pytest.raises(ValueError, match="weight"):
        Fh.conv2d_narrow(x, w)


def test_new_entry_points_are_declared_bound_and_registered():
    check_entry_points(NEW_SYMBOLS, "conv_narrow5.hip", 13)
    # the host-side mirror of the kernels' constants
    from tpgsr_amd import kernels as K
    src = open(os.path.join(ROOT, "tpgsr_amd", "csrc", "conv_narrow5.hip")).read()
    for name, value in (("kMaxCin", K.NARROW5_MAX_CIN), ("kMaxCout", K.NARROW5_MAX_COUT)):
        assert re.search(r"constexpr int %s = %d;" % (name, value), src), name
    assert K.narrow5_row(32, 3) == 2403 and K.narrow5_wgrad_blocks(1, 1, 1) == 1
    assert K.narrow5_wgrad_blocks(48, 32, 128) == K.NARROW5_WGRAD_BLOCKS <= 65536


@pytest.mark.parametrize("scale", [2, 4])
def test_cpu_input_runs_the_aten_path(scale):
    """the one deliberate stock-PyTorch path: a CPU tensor through the same parameter tensors, against the float64 restatement within the
    margin the fixture harness gives the reference's own float32 run (a quarter of the forward bound: 2.5e-5 of max(1, |y| max)); every
    parameter gets a gradient from autograd"""
    import make_golden_srcnn as GS
    from make_golden_next import generic_recipe
    from tpgsr_amd.model import srcnn
    net = srcnn.SRCNN(scale_factor=scale)
    sd = generic_recipe(net.state_dict(), GS.SEEDS[scale][1])
    net.load_state_dict(sd)
    x = torch.rand(2, 3, 12, 40, generator=torch.Generator().manual_seed(3))
    y = net(x)
    want = GS.srcnn_forward(GS.to64(sd), x.double(), scale)
    e = float((y.detach().double() - want).abs().max())
    assert tuple(y.shape) == (2, 3, 12 * scale, 40 * scale) and e <= 2.5e-5 * max(1.0, float(want.abs().max())), e
    y.sum().backward()
    assert all(p.grad is not None and float(p.grad.abs().max()) > 0 for p in net.parameters())
    assert "_eng" not in net.__dict__                                           # no engine was built for it
    # ... and nothing was launched: the C library's launch wrapper was never reached
    from tpgsr_amd import kernels as K
    seen, launch = [], K._launch
    K._launch = lambda name, *a: seen.append(name)
    try:
        net(x)
    finally:
        K._launch = launch
    assert seen == []
    # the CPU path takes what F.interpolate takes
    assert tuple(srcnn.SRCNN(scale_factor=1.5)(x).shape) == (2, 3, 18, 60)


IMPORTS = "from tpgsr_amd.model import srcnn"
CASES = r'''
nets = []
def srcnn_net(s, form):
    net = srcnn.SRCNN(scale_factor=s)
    net.set_tail_form(form)
    nets.append(net)
    return net

out["tail_default"] = Fh.NARROW5_DEFAULT_FORM
for form in ("narrow", "matrix", None):
    for s in (2, 4):
        r = train_case(lambda: srcnn_net(s, form), s, "mse")
        (pl,) = nets[-1]._engine()._plans.values()
        r["bwd_sid"] = [[o[0], o[3]] for o in pl["bwd"].ops]
        r["fwd_sid"] = [[o[0], o[3]] for o in pl["fwd"].ops]
        out[str(form) + str(s)] = r
for s in (2, 4):
    for form in ("narrow", "matrix", None):
        out["eval_%s_%d" % (form, s)] = eval_case(lambda: srcnn_net(s, form), s)
'''
EXTRA = r'''
# a non-integer factor is refused at the first device forward (the dry run takes the device path)
out["frac"] = err(lambda: srcnn.SRCNN(scale_factor=2.5)(torch.rand(1, 3, 4, 8)))
out["float_int"] = list(srcnn.SRCNN(scale_factor=2.0)(torch.rand(1, 3, 4, 8)).shape)
# the world-size refusal of the operator-level backbones
out["world"] = err(lambda: SRTrainStep(srcnn.SRCNN().train(), image_crit="mse", channels=3, world_size=2))
'''


@pytest.fixture(scope="module")
def rec():
    return record(IMPORTS, CASES, EXTRA)


SIDE = ("tpgsr_conv_wgrad", "tpgsr_wgrad_reduce_program", "tpgsr_conv5x5_narrow_bwd_weight", "tpgsr_reduce_partials")


@pytest.mark.timeout(600)
@pytest.mark.parametrize("scale", [2, 4])
def test_narrow_plan_of_the_train_step(rec, scale):
    r = rec[f"narrow{scale}"]
    assert r["key"] == ["(4, 3, 16, 64)", "True", "0", "x3"]
    assert r["sr"] == [4, 3, 16 * scale, 64 * scale] and r["pooled"] and r["sunk"] and not r["has_prior"] and r["scale"] == scale
    fwd, bwd = r["fwd"], r["bwd"]
    # forward: the up-sampling launch, conv1 and conv2 on the convolution route with a ReLU pass each, conv3 on the narrow launch
    assert fwd[:2] == ["tpgsr_nchw_to_nhwc", "tpgsr_resize_nearest_fwd"] and fwd[-2:] == ["tpgsr_conv5x5_narrow_fwd", "tpgsr_nhwc_to_nchw"]
    assert fwd.count("tpgsr_conv_fwd") == 2 and fwd.count("tpgsr_affine_act") == 2 and fwd.count("tpgsr_resize_nearest_fwd") == 1
    assert "join" not in fwd and all(sid == 0 for _, sid in r["fwd_sid"])
    # backward: conv3's data gradient on the narrow launch, conv2's on the convolution route, NONE for conv1 (the image needs no
    # gradient) and no nearest-neighbour backward
    assert bwd.count("tpgsr_conv5x5_narrow_bwd_data") == 1 and bwd.count("tpgsr_conv_fwd") == 1 and bwd.count("tpgsr_act_bwd") == 2
    assert "tpgsr_resize_nearest_bwd" not in bwd and bwd.count("tpgsr_nchw_to_nhwc") == 1 and "tpgsr_nhwc_to_nchw" not in bwd
    # weight gradients on stream 1: conv3's partial sums with their reduce into the two sinks, conv1's and conv2's slabs with the one
    # batched reduce; everything else on stream 0
    assert bwd.count("tpgsr_conv5x5_narrow_bwd_weight") == 1 and bwd.count("tpgsr_reduce_partials") == 1 and bwd.count("tpgsr_conv_wgrad") == 2
    assert bwd.count("tpgsr_wgrad_reduce_program") == 1 and "tpgsr_wgrad_reduce" not in bwd
    i = bwd.index("tpgsr_conv5x5_narrow_bwd_weight")
    assert bwd[i + 1:i + 4] == ["tpgsr_reduce_partials", "tpgsr_add", "tpgsr_add"]
    for name, sid in r["bwd_sid"]:
        if name in SIDE or name == "tpgsr_add":
            assert sid == 1, name
        elif name.startswith("tpgsr_"):
            assert sid == 0, name
    assert "fork" in bwd and bwd[-1] == "join"
    e = r["wrong_hr"]
    assert e and e[0] == "ValueError" and f"{scale}H, {scale}W" in e[1]


@pytest.mark.parametrize("scale", [2, 4])
def test_matrix_plan_takes_the_generic_route(rec, scale):
    r, n = rec[f"matrix{scale}"], rec[f"narrow{scale}"]
    fwd, bwd = r["fwd"], r["bwd"]
    assert not any("narrow" in name for name in fwd + bwd) and "tpgsr_reduce_partials" not in bwd
    assert fwd.count("tpgsr_conv_fwd") == 3 and bwd.count("tpgsr_conv_fwd") == 2 and bwd.count("tpgsr_conv_wgrad") == 3
    assert "tpgsr_resize_nearest_bwd" not in bwd and fwd.count("tpgsr_resize_nearest_fwd") == 1
    assert all(sid == 1 for name, sid in r["bwd_sid"] if name in SIDE) and r["sr"] == n["sr"] and r["scale"] == scale


@pytest.mark.parametrize("scale", [2, 4])
def test_default_plan_is_the_default_form(rec, scale):
    r = rec[f"None{scale}"]
    assert r["fwd"] == rec[rec["tail_default"] + str(scale)]["fwd"] and r["bwd"] == rec[rec["tail_default"] + str(scale)]["bwd"]


def test_mse_criterion_records_its_kernels(rec):
    """nn.MSELoss on three channels: the image-loss kernels next to the plan, the RGB prefixes of LR and HR by two strided copies"""
    for k in ("narrow2", "narrow4", "matrix2"):
        d = rec[k]["direct"]
        assert "tpgsr_image_loss_fwd" in d and "tpgsr_image_loss_bwd" in d, d
        assert "tpgsr_l1_loss_fwd" not in d and "tpgsr_charbonnier_loss_fwd" not in d
        assert d.count("tpgsr_copy_strided") == 2


def test_engine_scale_is_the_modules_factor(rec):
    assert rec["narrow2"]["scale"] == 2 and rec["narrow4"]["scale"] == 4


def test_evaluator_pass_takes_both_factors(rec):
    for s in (2, 4):
        for form in ("narrow", "matrix", None):
            r = rec[f"eval_{form}_{s}"]
            check_evaluator_case(r, s)
            narrow = (form or rec["tail_default"]) == "narrow"
            assert r["plan"].count("tpgsr_resize_nearest_fwd") == 1 and r["plan"].count("tpgsr_conv_fwd") == (2 if narrow else 3)
            assert r["plan"].count("tpgsr_conv5x5_narrow_fwd") == (1 if narrow else 0)


def test_non_integer_scale_is_refused_at_a_device_forward(rec):
    e = rec["frac"]
    assert e is not None and e[0] == "ValueError" and "integer factor" in e[1], e
    assert rec["float_int"] == [1, 3, 8, 16]


def test_gradient_exchange_stays_refused(rec):
    e = rec["world"]
    assert e is not None and e[0] == "NotImplementedError" and "gradient exchange" in e[1], e


@pytest.mark.parametrize("scale", [2, 4])
def test_fixtures_load_and_are_finite(scale):
    from test_srcnn_gpu import SRCNN as ARCH
    check_fixtures(ARCH, scale)
