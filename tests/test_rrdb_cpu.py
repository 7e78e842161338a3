"""CPU: `--arch esrgan` (RRDBNet x2 / x4) through the host layers -- constructor, state_dict layout against the reference's
(tests/golden/rrdb_layouts.json), initialisation, refusals, the C ABI of the new entry points, and plan recording in dry-run mode
(TPGSR_PLAN_DRYRUN=1, the pattern of tests/test_lapsrn_cpu.py) through `SRTrainStep` with image_crit="l1" in both forms of the dense
block and through the prior-free evaluator pass; the committed fixtures."""
import inspect
import json
import os
import sys

import pytest
import torch

from plain_arch_record import GOLD, ROOT, check_criterion_kernels, check_entry_points, check_evaluator_case, check_fixtures, record

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
    check_entry_points(NEW_SYMBOLS, "dense.hip", 13)


IMPORTS = "from tpgsr_amd.model import esrgan"
CASES = r'''
def rrdb_net(s, form=None):
    net = esrgan.RRDBNet(scale_factor=s, nb=NB)
    if form is not None:
        net.set_form(form)
    return net

out["default_form"] = Fh.DENSE_DEFAULT_FORM
for form in ("inplace", "composed"):
    for s in (2, 4):
        out[form + str(s)] = train_case(lambda: rrdb_net(s, form), s, "l1")
for s in (2, 4):
    out["eval_%d" % s] = eval_case(lambda: rrdb_net(s), s)
'''
EXTRA = r'''
# odd channel counts: form=None falls back to the composed form
del direct[:]
x = torch.rand(1, 5, 7, 6).requires_grad_(True)
ws = [torch.rand(2 if k < 4 else 6, 6 + 2 * k, 3, 3).requires_grad_(True) for k in range(5)]
y = Fh.dense_block(x, ws, None)
y.sum().backward()
out["odd"] = dict(direct=list(direct), y=list(y.shape))
'''


@pytest.fixture(scope="module")
def rec():
    return record(IMPORTS, CASES, EXTRA)


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
    check_criterion_kernels(rec, ("inplace2", "inplace4", "composed2"), "l1")


def test_evaluator_pass_takes_both_factors(rec):
    for s in (2, 4):
        r = rec[f"eval_{s}"]
        check_evaluator_case(r, s)
        want = "tpgsr_leaky_relu_window" if rec["default_form"] == "inplace" else "tpgsr_leaky_relu_fwd"
        assert r["plan"].count(want) >= 4 * 3 * NB


def test_odd_channel_counts_take_the_composed_form(rec):
    d = rec["odd"]
    assert d["y"] == [1, 5, 7, 6] and "tpgsr_leaky_relu_window" not in d["direct"] and d["direct"].count("tpgsr_scaled_add") == 2


@pytest.mark.parametrize("scale", [2, 4])
def test_fixtures_load_and_are_finite(scale):
    import plain_arch_common as P
    check_fixtures(P.RRDB, scale)
