"""GPU: `--arch srcnn` (SRCNN x2 / x4, nn.MSELoss on three channels) operator by operator on the HIP kernels and through `SRTrainStep` +
engine_functional.PlainSREngine against fixtures generated from the reference's own module (tests/golden/make_golden_srcnn.py), under
both forms of conv3 (SRCNN.set_tail_form: the direct 5x5 narrow-output kernels and the matrix route); recorded plans against the
operator-by-operator run on fresh inputs, hipGraph capture, the recorded step under the serial schedule (conv3's partial sums are reduced
into the arena on the side stream), the two-term policy, the prior-free evaluator pass, and the module API under autograd against the
step's gradient arena.

Bounds: BOUNDS of tests/plain_arch_common.py, unchanged, read through the `SRCNN` Arch below; the network-level bodies are there too --
forward images 1e-4 (of max(1, |y| max)), every parameter-gradient norm 5e-3 (check_param_grads), trajectory: loss 3e-4, clip norm 3e-3,
second loss 2e-2; recorded against operator by operator: SR bitwise, gradients 1e-6; x2 against x3: |dPSNR| < 1e-3 dB, loss 2e-5, clip
norm 2e-3.  The evaluator: SR 1e-4, |dPSNR| < 1e-5 dB and dSSIM < 1e-7 against the float64 restatement, identical strings.  The module API
against the arena: both run the same launches on the same inputs in the same order, so the gradients are held to the recorded-against-
eager bound 1e-6 (of the largest gradient element)."""
import dataclasses

import pytest
import torch

import plain_arch_common as P       # (puts tests/golden on the path)
import make_golden_srcnn as GS      # noqa: I100  (seeds and the float64 restatement only; the reference is not imported here)
from plain_arch_common import schedule  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

DEV = "cuda"
SCALES = [2, 4]
FORMS = ["narrow", "matrix"]      # conv3's form (SRCNN.set_tail_form): the network-level tests run both, whichever is the default


def _srcnn(scale, nb):
    from tpgsr_amd.model import srcnn
    return srcnn.SRCNN(scale_factor=scale)


# the forward records 14 launches (two layout changes, the up-sampling, three convolutions with their weight packing, two ReLUs), the
# backward 17: min_plan_ops sits below the eight operators of the forward
SRCNN = P.Arch(stem="srcnn", build=_srcnn, crit="mse", forward64=GS.srcnn_forward, ssim64=GS.ssim64, seeds={(None, s): v for s, v in GS.SEEDS.items()},
               n={None: GS.N}, n_store=GS.N_STORE, n_small=GS.N_SMALL, small_hw=GS.SMALL_HW, eval_n=GS.EVAL_N, eval_nb=None,
               eval_seeds=GS.EVAL_SEEDS, depths=(None,), nb_small=None, min_plan_ops=7, set_form=lambda net, form: net.set_tail_form(form))


def _with_form(form):
    """SRCNN whose constructor names conv3's form: the shared evaluator body builds its network without a `form` argument"""
    def build(scale, nb):
        net = _srcnn(scale, nb)
        net.set_tail_form(form)
        return net
    return dataclasses.replace(SRCNN, build=build, set_form=None)


# ---- 1. against the fixtures (x3) ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("scale", SCALES)
def test_srcnn_vs_reference_fixture(scale, form, golden_dir):
    """module(x) under autograd: the SR image, every parameter gradient for the seeded upstream gradient, the 12x40 eval forward"""
    net = P.check_vs_fixture(SRCNN, scale, None, golden_dir, form)
    assert net.tail_form == form and all(p.grad is not None for p in net.parameters())


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("scale", SCALES)
def test_srcnn_train_step_vs_reference_trajectory(scale, form, golden_dir):
    """two steps of the reference loop body (interfaces/super_resolution.py:409-424 with nn.MSELoss, torch.optim.Adam over
    model.parameters()) through SRTrainStep; all six tensors move"""
    P.check_trajectory(SRCNN, scale, None, golden_dir, form)


# ---- 2. recorded against operator by operator, capture + replay, the serial schedule, the two-term policy ---------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("scale", SCALES)
def test_recorded_plan_equals_operator_by_operator_run(scale, form):
    P.check_recorded_equals_eager(SRCNN, scale, form)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("scale", SCALES)
def test_capture_replay_equals_eager_steps(scale, form):
    """two replays are bitwise the eager twin's second and third step"""
    P.check_capture_replay(SRCNN, scale, form)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("scale", SCALES)
def test_recorded_step_equals_serial_schedule(scale, form, schedule):  # noqa: F811
    """conv3's partial sums are written, reduced and added into the arena on the side stream while the caller's stream moves on: the
    default schedule must give the bits of the SAME step replayed in recording order on one stream"""
    P.check_serial_schedule(SRCNN, scale, schedule, form)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("scale", SCALES)
def test_two_term_policy_holds_the_gates(scale, form):
    """the step's default policy x2 against x3 on the same batch and weights, with the bounds tests/test_policy_x2_gpu.py sets:
    |dPSNR| < 1e-3 dB, loss within 2e-5, gradient norm within 2e-3"""
    P.check_two_term_gates(SRCNN, scale, None, form)


# ---- 3. the prior-free pass of the evaluator --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("scale", SCALES)
def test_evaluator_pass(scale, form, golden_dir):
    """the recorded inference plan under either form of conv3 against the float64 restatement"""
    ev, net, lr = P.check_evaluator_pass(_with_form(form), scale, golden_dir)
    assert net.tail_form == form
    net.train()
    with pytest.raises(RuntimeError):
        ev.super_resolve(lr.to(DEV))


# ---- 4. the module API under autograd against the step's arena ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("scale", SCALES)
def test_module_autograd_equals_the_steps_arena(scale, form):
    """net(x).backward(dsr) hands every parameter the gradient the engine's recorded backward pass accumulates into the arena for the same
    input and upstream gradient; the SR images are bitwise equal"""
    from tpgsr_amd import kernels as K
    n = GS.N
    g = torch.Generator().manual_seed(97)
    lr = torch.rand(n, 3, 16, 64, generator=g).to(DEV)
    dsr = torch.randn(n, 3, 16 * scale, 64 * scale, generator=g).to(DEV)
    with K.policy("x3"):
        a = P.load(SRCNN, scale, None, form=form).train()
        y = a(lr)
        y.backward(dsr)
        b = P.load(SRCNN, scale, None, form=form).train()
        eng = b._engine()
        sr = eng.forward(lr, True)
        eng.arena.attach_grads()
        eng.arena.grad.zero_()
        assert eng.backward(tuple(lr.shape), sr, dsr) is None
        torch.cuda.synchronize()
    assert eng.record and torch.equal(sr, y.detach())
    ga, gb = dict(a.named_parameters()), dict(b.named_parameters())
    gmax = max(float(p.grad.abs().max()) for p in ga.values())
    for k in ga:
        d = float((ga[k].grad - gb[k].grad).abs().max())
        print(f"x{scale} {form} {k}: module API against the arena {d:.2e} (largest gradient element {gmax:.2e})")
        assert tuple(ga[k].grad.shape) == tuple(gb[k].grad.shape) and d <= SRCNN.bounds["rec_grad"] * gmax, (k, d)
