"""GPU: `--arch lapsrn` (LapSRN x2 / x4 + L1_Charbonnier_loss) operator by operator on the HIP kernels and through `SRTrainStep` +
engine_functional.PlainSREngine against fixtures generated from the reference's own module (tests/golden/make_golden_lapsrn.py); recorded
plans against the operator-by-operator run on fresh inputs, hipGraph capture, the step's two-term policy, the prior-free evaluator pass.

Bounds (the numbers live in BOUNDS of tests/plain_arch_common.py, read through the `LAPSRN` entry of its Arch table; the network-level
bodies are there too) -- for each quantity the one tests/test_plain_baselines_gpu.py applies to `srres`: forward images 1e-4 (of max(1,
|y| max)), every parameter-gradient norm 5e-3 (check_param_grads), trajectory: loss 3e-4, clip norm 3e-3, second loss 2e-2; recorded against operator by
operator: SR bitwise, gradients 1e-6; x2: |dPSNR| < 1e-3 dB, loss 2e-5, clip norm 2e-3.  The evaluator: SR 1e-4, |dPSNR| < 1e-5 dB and
dSSIM < 1e-7 against the float64 restatement, identical strings."""
import os

import numpy as np
import pytest
import torch

import plain_arch_common as P
from make_golden_lapsrn import CHANNELS, N_STORE, SEEDS, trained_names      # (seeds only; the reference is not imported here)
from oracle import tpgsr_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
N = 4
SCALES = [2, 4]


def load(scale, wseed=None):
    return P.load(P.LAPSRN, scale, None, wseed, dev=DEV)


def make_step(net, precision="x3"):
    return P.make_step(P.LAPSRN, net, precision)


# ---- 1. against the fixtures (x3) ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", SCALES)
def test_lapsrn_vs_reference_fixture(scale, golden_dir):
    """module(x) under autograd: the SR image, every parameter gradient for the seeded upstream gradient, the 12x40 eval forward"""
    net = P.check_vs_fixture(P.LAPSRN, scale, None, golden_dir)
    for n, p in net.named_parameters():      # x2: the second stage gets no gradient, as in the reference
        assert trained_names(scale)(n) or p.grad is None, n


@pytest.mark.parametrize("scale", SCALES)
def test_lapsrn_train_step_vs_reference_trajectory(scale, golden_dir):
    """two steps of the reference loop body (interfaces/super_resolution.py:409-424 with L1_Charbonnier_loss) through SRTrainStep; x2: the
    second stage's parameters are bit-identical after two steps"""
    P.check_trajectory(P.LAPSRN, scale, None, golden_dir)


# ---- 2. recorded against operator by operator, capture + replay, the two-term policy -------------------------------------------------
@pytest.mark.parametrize("scale", SCALES)
def test_recorded_plan_equals_operator_by_operator_run(scale):
    P.check_recorded_equals_eager(P.LAPSRN, scale)


@pytest.mark.parametrize("scale", SCALES)
def test_capture_replay_equals_eager_steps(scale):
    """two replays are bitwise the eager twin's second and third step (the channel-prefix launches inside the graph)"""
    P.check_capture_replay(P.LAPSRN, scale)


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
    B = P.LAPSRN.bounds
    assert dpsnr < B["x2_dpsnr"]
    assert abs(loss - t["loss"][0]) < B["x2_loss"] * t["loss"][0]
    assert abs(gn - t["gnorm"][0]) < B["x2_gnorm"] * t["gnorm"][0]


# ---- 3. the prior-free pass of the evaluator --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", SCALES)
def test_evaluator_pass(scale, golden_dir):
    ev, net, lr = P.check_evaluator_pass(P.LAPSRN, scale, golden_dir)
    net.train()
    with pytest.raises(RuntimeError):
        ev.super_resolve(lr.to(DEV))
