"""GPU: `--arch lapsrn` (LapSRN x2 / x4 + L1_Charbonnier_loss) operator by operator on the HIP kernels and through `SRTrainStep` +
engine_functional.PlainSREngine against fixtures generated from the reference's own module (tests/golden/make_golden_lapsrn.py); recorded
plans against the operator-by-operator run on fresh inputs, hipGraph capture, the step's two-term policy, the prior-free evaluator pass.

Bounds: for each quantity the one tests/test_plain_baselines_gpu.py applies to `srres` -- forward images 1e-4 (of max(1, |y| max)), every
parameter-gradient norm 5e-3 (check_param_grads), trajectory: loss 3e-4, clip norm 3e-3, second loss 2e-2; recorded against operator by
operator: SR bitwise, gradients 1e-6; x2: |dPSNR| < 1e-3 dB, loss 2e-5, clip norm 2e-3.  The evaluator: SR 1e-4, |dPSNR| < 1e-5 dB and
dSSIM < 1e-7 against the float64 restatement, identical strings."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_golden_lapsrn import (CHANNELS, EVAL_N, EVAL_SEEDS, N_SMALL, N_STORE, SEEDS, SMALL_HW, lapsrn_forward, ssim64, to64,  # noqa: E402
                                trained_names)      # (seeds and the float64 restatement only; the reference is not imported here)
from make_golden_next import generic_recipe  # noqa: E402
from oracle import tpgsr_oracle as O  # noqa: E402
from test_tl_cascade_gpu import check_param_grads  # noqa: E402  (the per-parameter rule of tests/test_next_models_gpu.py)

DEV = "cuda"
N = 4
SCALES = [2, 4]


def load(scale, wseed=None):
    from tpgsr_amd.model import lapsrn
    net = lapsrn.LapSRN(scale_factor=scale, width=128, height=32, STN=False)
    net.load_state_dict(generic_recipe(net.state_dict(), SEEDS[scale][1] if wseed is None else wseed), strict=True)
    return net.to(DEV)


def make_step(net, precision="x3"):
    from tpgsr_amd.interfaces.super_resolution import SRTrainStep
    return SRTrainStep(net, image_crit="l1_charbonnier", channels=CHANNELS, precision=precision)


# ---- 1. against the fixtures (x3) ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", SCALES)
def test_lapsrn_vs_reference_fixture(scale, golden_dir):
    """module(x) under autograd: the SR image, every parameter gradient for the seeded upstream gradient, the 12x40 eval forward"""
    from tpgsr_amd import kernels as K
    g = np.load(os.path.join(golden_dir, f"lapsrn_x{scale}.npz"))
    dseed, wseed, gseed, sseed = SEEDS[scale]
    assert [int(s) for s in g["seeds"]] == [dseed, wseed, gseed, sseed]
    x = O.synthetic_batch(N, dseed, scale=scale)[0][:, :CHANNELS].contiguous().to(DEV)
    with K.policy("x3"):
        net = load(scale).train()
        y = net(x)
        yref = torch.tensor(g["y"])
        sc = max(1.0, float(yref.abs().max()))
        err = (y.detach().cpu()[:N_STORE[scale]] - yref).abs().max().item()
        gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(gseed))
        (y * gy.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        print(f"x{scale}: train fwd max err {err:.2e} (|y| max {float(yref.abs().max()):.2f})")
        assert tuple(y.shape) == (N, CHANNELS, 16 * scale, 64 * scale) and err < 1e-4 * sc
        live = np.array([trained_names(scale)(str(n)) for n in g["grad_names"]])
        check_param_grads(f"x{scale}", net, g["grad_names"][live], g["grad_norms"][live], g["grad_heads"][live])
        for n, p in net.named_parameters():      # x2: the second stage gets no gradient, as in the reference
            assert trained_names(scale)(n) or p.grad is None, n
        net2 = load(scale).eval()
        with torch.no_grad():
            xs = O.synthetic_batch(N_SMALL, sseed, lr_hw=SMALL_HW, scale=scale)[0][:, :CHANNELS].contiguous().to(DEV)
            ys = net2(xs)                                   # fully convolutional: 12x40 is no multiple of the 16-row / 64-column tiles
    e = (ys.cpu() - torch.tensor(g["y_small"])).abs().max().item()
    print(f"   eval 12x40 fwd max err {e:.2e}")
    assert tuple(ys.shape) == g["y_small"].shape and e < 1e-4 * max(1.0, float(np.abs(g["y_small"]).max()))


@pytest.mark.parametrize("scale", SCALES)
def test_lapsrn_train_step_vs_reference_trajectory(scale, golden_dir):
    """two steps of the reference loop body (interfaces/super_resolution.py:409-424 with L1_Charbonnier_loss) through SRTrainStep"""
    from tpgsr_amd.engine_functional import PlainSREngine
    t = np.load(os.path.join(golden_dir, f"train_lapsrn_x{scale}.npz"))
    lr, hr = [a.to(DEV) for a in O.synthetic_batch(N, SEEDS[scale][0], scale=scale)]
    net = load(scale).train()
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    ts = make_step(net)
    losses, gns = [], []
    for step in range(2):
        loss = ts.step(lr, hr)
        torch.cuda.synchronize()
        losses.append(loss.item())
        gns.append(ts.opt.grad_norm(net).item())
        if step == 0:
            ref = torch.tensor(t["sr_step0"])
            e = (ts.last_sr.cpu()[:N_STORE[scale]] - ref).abs().max().item()
            print(f"   x{scale}: sr_step0 max err {e:.2e}")
            assert tuple(ts.last_sr.shape) == (N, CHANNELS, 16 * scale, 64 * scale) and e < 1e-4 * max(1.0, float(ref.abs().max()))
    print(f"x{scale} losses {losses} vs {t['loss']}; clip norms {gns} vs {t['gnorm']}")
    assert abs(losses[0] - t["loss"][0]) < 3e-4 * t["loss"][0]
    assert abs(gns[0] - t["gnorm"][0]) < 3e-3 * t["gnorm"][0]
    assert abs(losses[1] - t["loss"][1]) < 2e-2 * t["loss"][1]
    eng = net._engine()
    assert isinstance(eng, PlainSREngine) and eng.record and eng.scale == scale and len(eng._plans) == 1
    after = net.state_dict()
    for k in before:
        if trained_names(scale)(k):
            assert not torch.equal(before[k], after[k]), k
        else:      # x2: the second stage's parameters are bit-identical after two steps
            assert torch.equal(before[k], after[k]), k


# ---- 2. recorded against operator by operator, capture + replay, the two-term policy -------------------------------------------------
def _passes(scale, record, n_pass=3):
    from tpgsr_amd import kernels as K
    net = load(scale).train()
    eng = net._engine()
    eng.record = record
    g = torch.Generator().manual_seed(93)
    outs = []
    with K.policy("x3"):
        for i in range(n_pass):
            lr = torch.rand(N, CHANNELS, 16, 64, generator=g).to(DEV)
            dsr = torch.randn(N, CHANNELS, 16 * scale, 64 * scale, generator=g).to(DEV)
            sr = eng.forward(lr, True, slot=i % 2)
            eng.arena.attach_grads()
            eng.arena.grad.zero_()
            assert eng.backward(tuple(lr.shape), sr, dsr, slot=i % 2) is None
            torch.cuda.synchronize()
            outs.append(dict(sr=sr.clone(), grad=eng.arena.grad.clone()))
    return outs, eng


@pytest.mark.parametrize("scale", SCALES)
def test_recorded_plan_equals_operator_by_operator_run(scale):
    rec, eng = _passes(scale, True)
    ref, _ = _passes(scale, False)
    assert len(eng._plans) == 2 and all(len(pl["fwd"]) > 20 and len(pl["bwd"]) > 20 for pl in eng._plans.values())
    for i, (a, b) in enumerate(zip(rec, ref)):
        assert torch.equal(a["sr"], b["sr"]), (i, float((a["sr"] - b["sr"]).abs().max()))
        d = (a["grad"] - b["grad"]).abs().max().item()
        assert d <= 1e-6 * b["grad"].abs().max().item(), (i, d)


@pytest.mark.parametrize("scale", SCALES)
def test_capture_replay_equals_eager_steps(scale):
    """two replays are bitwise the eager twin's second and third step (the channel-prefix launches inside the graph)"""
    lr, hr = [a.to(DEV) for a in O.synthetic_batch(N, SEEDS[scale][0], scale=scale)]
    net_a, net_b = load(scale).train(), load(scale).train()
    ea, eb = make_step(net_a, None), make_step(net_b, None)
    eb.capture(lr, hr, warmup=1)
    la = [ea.step(lr, hr).item() for _ in range(3)]
    lb = [eb.replay().item() for _ in range(2)]
    torch.cuda.synchronize()
    print(la, lb)
    assert lb[0] == la[1] and lb[1] == la[2]
    assert torch.equal(ea.pool.flat, eb.pool.flat)
    assert torch.equal(ea.last_sr, eb.last_sr)


def test_two_term_policy_holds_the_gates(golden_dir):
    """the step's default policy x2 at x4 against the reference fixture, with the bounds tests/test_policy_x2_gpu.py sets: |dPSNR| < 1e-3 dB,
    loss within 2e-5, gradient norm within 2e-3"""
    scale = 4
    t = np.load(os.path.join(golden_dir, f"train_lapsrn_x{scale}.npz"))
    lr, hr = [a.to(DEV) for a in O.synthetic_batch(N, SEEDS[scale][0], scale=scale)]
    net = load(scale).train()
    ts = make_step(net, precision="x2")
    loss = ts.step(lr, hr).item()
    torch.cuda.synchronize()
    gn = ts.opt.grad_norm(net).item()
    ref, k = torch.tensor(t["sr_step0"]), N_STORE[scale]
    hr_k = hr.cpu()[:k, :CHANNELS]
    dpsnr = abs(float(O.calculate_psnr(ts.last_sr.cpu()[:k], hr_k)) - float(O.calculate_psnr(ref, hr_k)))
    print(f"x{scale} x2: loss {loss:.6f} vs {t['loss'][0]:.6f}; |dPSNR| {dpsnr:.3e} dB; clip norm {gn:.5f} vs {t['gnorm'][0]:.5f}")
    assert dpsnr < 1e-3
    assert abs(loss - t["loss"][0]) < 2e-5 * t["loss"][0]
    assert abs(gn - t["gnorm"][0]) < 2e-3 * t["gnorm"][0]


# ---- 3. the prior-free pass of the evaluator --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", SCALES)
def test_evaluator_pass(scale, golden_dir):
    from tpgsr_amd.interfaces.super_resolution import TextSREvaluator
    from tpgsr_amd.model.crnn import crnn
    g = np.load(os.path.join(golden_dir, f"lapsrn_x{scale}.npz"))
    lr, hr = O.synthetic_batch(EVAL_N, int(g["eval_seed"]), scale=scale)
    net = load(scale, EVAL_SEEDS[scale]).eval()
    sd = generic_recipe(net.state_dict(), EVAL_SEEDS[scale])
    rec = crnn.CRNN(32, 1, 37, 256)
    rec.load_state_dict(O.recipe_state_dict(O.crnn_spec(), EVAL_SEEDS["rec"]))
    ev = TextSREvaluator([net], None, recognizer=rec.to(DEV).eval(), channels=CHANNELS)
    labels = ["abc", "y3", "", "hello", "y3y3", "zz9"]
    out = ev.eval_batch(lr.to(DEV), hr.to(DEV), labels)
    torch.cuda.synchronize()
    with torch.no_grad():
        want = lapsrn_forward(to64({k: v.cpu() for k, v in sd.items()}), lr[:, :CHANNELS].double(), scale)
        hr64 = hr[:, :CHANNELS].double()
        psnr64, ssim_64 = float(O.calculate_psnr(want, hr64)), float(ssim64(want, hr64))
    assert len(out["images_sr"]) == 1 and out["priors"] == []
    sr = out["images_sr"][0]
    e = (sr.cpu().double() - want).abs().max().item()
    dp, ds = abs(float(out["psnr"]) - psnr64), abs(float(out["ssim"]) - ssim_64)
    print(f"x{scale}: SR max err {e:.2e}; psnr {float(out['psnr']):.6f} vs {psnr64:.6f} (|d| {dp:.2e} dB); ssim {float(out['ssim']):.8f} vs "
          f"{ssim_64:.8f} (|d| {ds:.2e})")
    assert tuple(sr.shape) == (EVAL_N, CHANNELS, 16 * scale, 64 * scale) and e < 1e-4 * max(1.0, float(want.abs().max()))
    assert dp < 1e-5
    assert ds < 1e-7
    strings = {k: [str(s) for s in g["eval_" + k]] for k in ("sr", "lr", "hr")}
    assert out["pred_sr"] == strings["sr"] and out["pred_lr"] == strings["lr"] and out["pred_hr"] == strings["hr"]
    assert out["n_correct_sr"] == sum(a == b for a, b in zip(strings["sr"], labels))
    # the HR grid follows the engine's factor: the other factor's HR batch is refused
    other = O.synthetic_batch(EVAL_N, int(g["eval_seed"]), scale=6 - scale)[1]
    with pytest.raises(ValueError):
        ev.eval_batch(lr.to(DEV), other.to(DEV))
    net.train()
    with pytest.raises(RuntimeError):
        ev.super_resolve(lr.to(DEV))
