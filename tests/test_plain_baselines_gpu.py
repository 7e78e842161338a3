"""GPU: the prior-free baselines (`--arch srres | rdn | vdsr | bicubic`) -- SRResNet / RDN / VDSR operator by operator on the HIP kernels
and through `SRTrainStep` + engine_functional.PlainSREngine against fixtures generated from the reference's own modules
(tests/golden/make_golden_plain.py); recorded plans against the operator-by-operator run on fresh inputs, hipGraph capture, the step's
default two-term policy; tpgsr_bicubic_upsample against float64 F.interpolate; the prior-free pass of TextSREvaluator."""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from kernel_table import KCase, _gen, check_case  # noqa: E402
from make_golden_next import generic_recipe  # noqa: E402  (the weight recipe only; the reference is not imported here)
from make_golden_plain import (BACKBONES, CHANNELS, CRIT, EVAL_CHANNELS, EVAL_SEEDS, N_SMALL, SEEDS, SMALL_HW, plain_forward,  # noqa: E402
                               to64)      # (names, criteria, seeds and the float64 restatement only)
from oracle import tpgsr_oracle as O  # noqa: E402
from test_tl_cascade_gpu import check_param_grads  # noqa: E402  (the per-parameter rule of tests/test_next_models_gpu.py)

DEV = "cuda"
N = 4


def build_backbone(name):
    from tpgsr_amd.model import rdn, srresnet, vdsr
    if name == "srres":
        return srresnet.SRResNet(scale_factor=2, width=128, height=32, STN=False, mask=True)
    if name == "rdn":
        return rdn.RDN(scale_factor=2)
    return vdsr.VDSR(scale_factor=2, width=128, height=32, STN=False)


def load(name, wseed=None):
    net = build_backbone(name)
    net.load_state_dict(generic_recipe(net.state_dict(), SEEDS[name][1] if wseed is None else wseed), strict=True)
    return net.to(DEV)


def make_step(name, net, precision="x3"):
    from tpgsr_amd.interfaces.super_resolution import SRTrainStep
    return SRTrainStep(net, image_crit=CRIT[name], channels=None if name == "srres" else CHANNELS[name], precision=precision)


# ---- 1. per backbone against its fixture (x3) --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BACKBONES)
def test_plain_backbone_vs_reference_fixture(name, golden_dir):
    """module(x) under autograd: eval forward, train forward, every parameter gradient, running buffers, the 12x40 eval forward -- the
    bounds tests/test_next_models_gpu.py asserts for the `_TL` sibling"""
    from tpgsr_amd import kernels as K
    g = np.load(os.path.join(golden_dir, f"plain_{name}.npz"))
    dseed, wseed, gseed, sseed = SEEDS[name]
    C = CHANNELS[name]
    assert [int(s) for s in g["seeds"]] == [dseed, wseed, gseed, sseed]
    x = O.synthetic_batch(N, dseed)[0][:, :C].contiguous().to(DEV)
    with K.policy("x3"):
        net = load(name).train()
        y = net(x)
        yref = torch.tensor(g["y"])
        scale = max(1.0, float(yref.abs().max()))
        err = (y.detach().cpu() - yref).abs().max().item()
        gy = torch.randn(yref.shape, generator=torch.Generator().manual_seed(gseed))
        (y * gy.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        print(f"{name}: train fwd max err {err:.2e} (|y| max {scale:.2f})")
        assert y.shape == yref.shape and err < 1e-4 * scale
        check_param_grads(name, net, g["grad_names"], g["grad_norms"], g["grad_heads"])
        if len(g["running_cat"]) > 1:
            cat = torch.cat([v.detach().cpu().reshape(-1).float() for k, v in net.state_dict().items() if "running_" in k])
            e = (cat - torch.tensor(g["running_cat"])).abs().max().item()
            print(f"   running buffers max err {e:.2e}")
            assert e < 2e-4
            assert all(int(v) == 1 for k, v in net.state_dict().items() if k.endswith("num_batches_tracked"))
        net2 = load(name).eval()
        with torch.no_grad():
            ye = net2(x)
            xs = O.synthetic_batch(N_SMALL, sseed, lr_hw=SMALL_HW)[0][:, :C].contiguous().to(DEV)
            ys = net2(xs)                                   # fully convolutional: 12x40 is no multiple of the 16-row / 64-column tiles
    for tag, got, want in (("eval", ye, g["y_eval"]), ("eval 12x40", ys, g["y_small"])):
        e = (got.cpu() - torch.tensor(want)).abs().max().item()
        print(f"   {tag} fwd max err {e:.2e}")
        assert tuple(got.shape) == want.shape and e < 1e-4 * max(1.0, float(np.abs(want).max()))


@pytest.mark.parametrize("name", BACKBONES)
def test_plain_backbone_train_step_vs_reference_trajectory(name, golden_dir):
    """two steps of the reference loop body (interfaces/super_resolution.py:409-424) through SRTrainStep: the bounds of
    tests/test_tl_cascade_gpu.py run_against_fixture"""
    from tpgsr_amd.engine_functional import PlainSREngine
    t = np.load(os.path.join(golden_dir, f"train_plain_{name}.npz"))
    lr, hr = [a.to(DEV) for a in O.synthetic_batch(N, SEEDS[name][0])]
    net = load(name).train()
    ts = make_step(name, net)
    losses, gns = [], []
    for step in range(2):
        loss = ts.step(lr, hr)
        torch.cuda.synchronize()
        losses.append(loss.item())
        gns.append(ts.opt.grad_norm(net).item())
        if step == 0:
            ref = torch.tensor(t["sr_step0"])
            e = (ts.last_sr.cpu() - ref).abs().max().item()
            print(f"   {name}: sr_step0 max err {e:.2e}")
            assert ts.last_sr.shape == ref.shape and e < 1e-4 * max(1.0, float(ref.abs().max()))
    print(f"{name} losses {losses} vs {t['loss']}; clip norms {gns} vs {t['gnorm']}")
    assert abs(losses[0] - t["loss"][0]) < 3e-4 * t["loss"][0]
    assert abs(gns[0] - t["gnorm"][0]) < 3e-3 * t["gnorm"][0]
    assert abs(losses[1] - t["loss"][1]) < 2e-2 * t["loss"][1]
    eng = net._engine()
    assert isinstance(eng, PlainSREngine) and eng.record and len(eng._plans) == 1
    a, b = ts.pool.ranges[id(net)]
    assert ts.pool.flat[a:b].data_ptr() == eng.arena.flat.data_ptr()


# ---- 2. srres: recorded against operator by operator, capture + replay, the two-term policy ------------------------------------------
def _passes(record, n_pass=3):
    from tpgsr_amd import kernels as K
    net = load("srres").train()
    eng = net._engine()
    eng.record = record
    g = torch.Generator().manual_seed(92)
    outs = []
    with K.policy("x3"):
        for i in range(n_pass):
            lr = torch.rand(N, 4, 16, 64, generator=g).to(DEV)
            dsr = torch.randn(N, 4, 32, 128, generator=g).to(DEV)
            sr = eng.forward(lr, True, slot=i % 2)
            eng.arena.attach_grads()
            eng.arena.grad.zero_()
            assert eng.backward(tuple(lr.shape), sr, dsr, slot=i % 2) is None
            torch.cuda.synchronize()
            outs.append(dict(sr=sr.clone(), grad=eng.arena.grad.clone()))
    eng.flush_counters()
    return outs, {k: v.clone() for k, v in net.named_buffers()}, eng


def test_recorded_plan_equals_operator_by_operator_run():
    rec, bufs_r, eng = _passes(True)
    ref, bufs_e, _ = _passes(False)
    assert len(eng._plans) == 2 and all(len(pl["fwd"]) > 20 and len(pl["bwd"]) > 20 for pl in eng._plans.values())
    for i, (a, b) in enumerate(zip(rec, ref)):
        assert torch.equal(a["sr"], b["sr"]), (i, float((a["sr"] - b["sr"]).abs().max()))
        d = (a["grad"] - b["grad"]).abs().max().item()
        assert d <= 1e-6 * b["grad"].abs().max().item(), (i, d)
    assert bufs_e
    for k in bufs_e:
        assert torch.equal(bufs_r[k].float(), bufs_e[k].float()), k


@pytest.mark.parametrize("name", ["srres", "rdn"])
def test_capture_replay_equals_eager_steps(name):
    """two replays are bitwise the eager twin's second and third step (rdn: with the channel-prefix launches inside the graph)"""
    lr, hr = [a.to(DEV) for a in O.synthetic_batch(N, SEEDS[name][0])]
    net_a, net_b = load(name).train(), load(name).train()
    ea, eb = make_step(name, net_a, None), make_step(name, net_b, None)
    eb.capture(lr, hr, warmup=1)
    la = [ea.step(lr, hr).item() for _ in range(3)]
    lb = [eb.replay().item() for _ in range(2)]
    torch.cuda.synchronize()
    print(la, lb)
    assert lb[0] == la[1] and lb[1] == la[2]
    assert torch.equal(ea.pool.flat, eb.pool.flat)
    assert torch.equal(ea.last_sr, eb.last_sr)


def test_two_term_policy_holds_the_gates(golden_dir):
    """the step's default policy x2 against the reference fixture, with the bounds tests/test_policy_x2_gpu.py sets: |dPSNR| < 1e-3 dB, loss
    within 2e-5, gradient norm within 2e-3"""
    name = "srres"
    t = np.load(os.path.join(golden_dir, f"train_plain_{name}.npz"))
    lr, hr = [a.to(DEV) for a in O.synthetic_batch(N, SEEDS[name][0])]
    net = load(name).train()
    ts = make_step(name, net, precision="x2")
    loss = ts.step(lr, hr).item()
    torch.cuda.synchronize()
    gn = ts.opt.grad_norm(net).item()
    ref = torch.tensor(t["sr_step0"])
    dpsnr = abs(float(O.calculate_psnr(ts.last_sr.cpu(), hr.cpu())) - float(O.calculate_psnr(ref, hr.cpu())))
    print(f"{name} x2: loss {loss:.6f} vs {t['loss'][0]:.6f}; |dPSNR| {dpsnr:.3e} dB; clip norm {gn:.5f} vs {t['gnorm'][0]:.5f}")
    assert dpsnr < 1e-3
    assert abs(loss - t["loss"][0]) < 2e-5 * t["loss"][0]
    assert abs(gn - t["gnorm"][0]) < 2e-3 * t["gnorm"][0]


# ---- 3. tpgsr_bicubic_upsample against float64 F.interpolate (the rule of tests/kernel_table.py) ----------------------------------------
def _bu_make(shape, seed):
    return {"x": torch.rand(*shape, generator=_gen("bicubic_upsample", shape, seed)) * 2 - 0.5}


def _bu_ref(d, C, s):
    return {"y": F.interpolate(d["x"][:, :C], scale_factor=s, mode="bicubic", align_corners=True)}


def _bu_gpu(d, C, s):
    from tpgsr_amd import kernels as K
    x = d["x"]
    n, ctot, h, w = x.shape
    y = torch.full((n, C, h * s, w * s), float("nan"), device=DEV)
    K.bicubic_upsample(x, n, ctot, C, h, w, s, y)
    return {"y": y}


#            (N, Ctot, H, W), C, scale
BU_SHAPES = [((2, 4, 16, 64), 4, 2), ((1, 4, 5, 7), 3, 2), ((1, 2, 4, 6), 2, 3), ((1, 1, 1, 1), 1, 2), ((1, 1, 1, 9), 1, 2)]
BU_CASES = [KCase("bicubic_upsample", f"{'x'.join(map(str, shape))}-c{C}-s{s}", lambda seed, shape=shape: _bu_make(shape, seed),
                  lambda d, C=C, s=s: _bu_ref(d, C, s), lambda d, C=C, s=s: _bu_gpu(d, C, s)) for shape, C, s in BU_SHAPES]


@pytest.mark.parametrize("case", BU_CASES, ids=[c.id for c in BU_CASES])
def test_bicubic_upsample_vs_float64(case):
    check_case(case, {})


def test_bicubic_module_and_refused_arguments():
    from tpgsr_amd import kernels as K
    from tpgsr_amd._lib import TpgsrKernelError
    from tpgsr_amd.model.bicubic import BICUBIC
    x = torch.rand(2, 4, 16, 64, generator=torch.Generator().manual_seed(3)).to(DEV)
    y = BICUBIC(scale_factor=2)(x)
    want = F.interpolate(x.cpu().double(), scale_factor=2, mode="bicubic", align_corners=True)
    # 16 products of weights with sum |wy| sum |wx| <= 1.5625 and |x| < 1 accumulated in fp32, one rounding in each tap fraction
    assert y.shape == (2, 4, 32, 128) and (y.cpu().double() - want).abs().max().item() < 16 * 1.5625 * 2.0 ** -24 * 4
    assert torch.equal(BICUBIC(2)(x, channels=3), y[:, :3])                       # the channel prefix without a copy of the input
    assert torch.equal(BICUBIC(1)(x), x)                                          # scale 1: every tap fraction is 0
    y = torch.empty(2, 4, 32, 128, device=DEV)
    for args, word in (((x, 2, 4, 4, 16, 64, 0, y), "scale"), ((x, 2, 4, 5, 16, 64, 2, y), "C <= Ctot"), ((x, 2, 4, 0, 16, 64, 2, y), "C <= Ctot"),
                       ((x, 0, 4, 4, 16, 64, 2, y), "at least 1"), ((x, 2, 4, 4, 16, 0, 2, y), "at least 1"),
                       ((x, 2, 4, 4, 16, 1 << 30, 4, y), "2^31"), ((x, 1 << 20, 4, 4, 1 << 20, 64, 2, y), "grid limit")):
        with pytest.raises(TpgsrKernelError, match=re.escape(word)):
            K.bicubic_upsample(*args)
    with pytest.raises(NotImplementedError):
        BICUBIC(scale_factor=1.5)


# ---- 4. the prior-free pass of the evaluator ------------------------------------------------------------------------------------------
def _eval_case(name):
    """-> (model on the GPU in eval mode, float64 SR function on the CPU)"""
    from tpgsr_amd.model import tsrn
    from tpgsr_amd.model.bicubic import BICUBIC
    if name == "srres":
        net = load("srres", EVAL_SEEDS["srres"]).eval()
        sd = generic_recipe(build_backbone("srres").state_dict(), EVAL_SEEDS["srres"])
        return net, lambda lr: plain_forward("srres", to64(sd), lr.double(), False)
    if name == "tsrn":
        sd = O.recipe_state_dict(O.tsrn_spec(STN=False, mask=True), EVAL_SEEDS["tsrn"])
        net = tsrn.TSRN(scale_factor=2, width=128, height=32, STN=False, mask=True)
        net.load_state_dict(sd)
        return net.to(DEV).eval(), lambda lr: O.tsrn_forward(O.as_params(to64(sd), False), lr.double(), training=False, stn=False)
    if name == "rdn":      # channels=3: the network sees the RGB prefix, PSNR / SSIM the RGB planes of HR
        net = load("rdn", EVAL_SEEDS["rdn"]).eval()
        sd = generic_recipe(build_backbone("rdn").state_dict(), EVAL_SEEDS["rdn"])
        return net, lambda lr: plain_forward("rdn", to64(sd), lr[:, :3].double(), False)
    return BICUBIC(scale_factor=2), lambda lr: F.interpolate(lr.double(), scale_factor=2, mode="bicubic", align_corners=True)


@pytest.mark.parametrize("name", ["srres", "tsrn", "bicubic", "rdn"])
def test_prior_free_evaluator_pass(name, golden_dir):
    from tpgsr_amd.interfaces.super_resolution import TextSREvaluator
    from tpgsr_amd.model.crnn import crnn
    fx = json.load(open(os.path.join(golden_dir, "plain_eval.json")))
    assert fx["weight_seeds"] == EVAL_SEEDS
    lr, hr = O.synthetic_batch(fx["n"], fx["data_seed"])
    model, sr64 = _eval_case(name)
    rec = crnn.CRNN(32, 1, 37, 256)
    rec.load_state_dict(O.recipe_state_dict(O.crnn_spec(), EVAL_SEEDS["rec"]))
    ev = TextSREvaluator([model], None, recognizer=rec.to(DEV).eval(), channels=EVAL_CHANNELS[name])
    labels = ["abc", "y3", "", "hello", "y3y3", "zz9"]
    out = ev.eval_batch(lr.to(DEV), hr.to(DEV), labels)
    torch.cuda.synchronize()
    with torch.no_grad():
        want = sr64(lr)
    assert len(out["images_sr"]) == 1 and out["priors"] == []
    e = (out["images_sr"][0].cpu().double() - want).abs().max().item()
    print(f"{name}: SR max err {e:.2e}; psnr {float(out['psnr']):.5f} vs {fx['psnr'][name]:.5f}; ssim {float(out['ssim']):.7f} vs {fx['ssim'][name]:.7f}")
    assert e < 1e-4 * max(1.0, float(want.abs().max()))
    assert abs(float(out["psnr"]) - fx["psnr"][name]) < 1e-3
    assert abs(float(out["ssim"]) - fx["ssim"][name]) < 1e-5
    assert out["pred_sr"] == fx["strings"]["sr_" + name] and out["pred_lr"] == fx["strings"]["lr"] and out["pred_hr"] == fx["strings"]["hr"]
    assert out["n_correct_sr"] == sum(a == b for a, b in zip(fx["strings"]["sr_" + name], labels))
    if name == "srres":
        model.train()
        with pytest.raises(RuntimeError):
            ev.super_resolve(lr.to(DEV))
