"""GPU: `--arch esrgan` (RRDBNet x2 / x4, nn.L1Loss) -- functional.dense_block in both forms, the module operator by operator and through
`SRTrainStep` + engine_functional.PlainSREngine against fixtures generated from the reference's own module
(tests/golden/make_golden_rrdb.py); recorded plans against the operator-by-operator run on fresh inputs, hipGraph capture, the recorded
step under the serial schedule (the side-stream reads of the in-place gradient buffer), the two-term policy, the prior-free evaluator pass.

Bounds (the numbers live in BOUNDS of tests/plain_arch_common.py, read through the `RRDB` entry of its Arch table; the network-level
bodies are there too): forward images 1e-4 (of max(1, |y| max)), every parameter-gradient norm 5e-3 (check_param_grads), trajectory: loss 3e-4, clip norm 3e-3, second loss 2e-2; recorded against operator by operator: SR
bitwise, gradients 1e-6; x2 against x3: |dPSNR| < 1e-3 dB, loss 2e-5, clip norm 2e-3.  The evaluator: SR 1e-4, |dPSNR| < 1e-5 dB and
dSSIM < 1e-7 against the float64 restatement, identical strings (the float64 SSIM runs over the reference's float32-built window taps,
golden_plain_arch.ssim_window: taps built in float64 and rounded afterwards move the mean SSIM of the x2 batch by 1.1e-7 on their own).
dense_block: the in-place form against the composed one within 1e-6
(of the composed result's largest magnitude) under the default policy x3; both against float64 autograd under the `arith` rule of
tests/kernel_table.py (e_gpu <= 4 * e_ref32 + 4 * 2^-24) under policy f32 -- the rule measures float32 arithmetic against float32
arithmetic, and f32 is the policy whose products are float32 (the split-bf16 policies have limits of their own: CONV_LIMITS of
tests/test_functional_ops_gpu.py)."""
import pytest
import torch
import torch.nn.functional as F

import plain_arch_common as P
from kernel_table import FLOOR, _gen, err
from plain_arch_common import schedule  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

DEV = "cuda"
SCALES = [2, 4]
DEPTHS = [2, 23]


def load(scale, nb, wseed=None):
    return P.load(P.RRDB, scale, nb, wseed, dev=DEV)


def make_step(net, precision="x3"):
    return P.make_step(P.RRDB, net, precision)


# ---- 0. functional.dense_block ---------------------------------------------------------------------------------------------------------
NF, GC = 64, 32


def _block_inputs(hw):
    g = _gen("dense_block", hw)
    x = torch.randn(2, hw[0], hw[1], NF, generator=g)
    ws = [torch.randn(GC if k < 4 else NF, NF + k * GC, 3, 3, generator=g) / (3 * (NF + k * GC) ** 0.5) for k in range(5)]
    bs = [0.1 * torch.randn(GC if k < 4 else NF, generator=g) for k in range(5)]
    gy = torch.randn(2, hw[0], hw[1], NF, generator=g)
    return x, ws, bs, gy


def _block_ref(x, ws, bs, gy, dtype):
    """stock PyTorch autograd in `dtype` (NHWC in, NHWC out): y, dx, dw1..5, db1..5"""
    x = x.to(dtype).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    ws = [w.detach().clone().to(dtype).requires_grad_(True) for w in ws]      # (copies: `to` of the same dtype returns its argument)
    bs = [b.detach().clone().to(dtype).requires_grad_(True) for b in bs]
    feats = [x]
    for k in range(4):
        feats.append(F.leaky_relu(F.conv2d(torch.cat(feats, 1), ws[k], bs[k], padding=1), 0.2))
    y = F.conv2d(torch.cat(feats, 1), ws[4], bs[4], padding=1) * torch.tensor(0.2, dtype=torch.float32).to(dtype) + x
    (y * gy.to(dtype).permute(0, 3, 1, 2)).sum().backward()
    return [y.detach().permute(0, 2, 3, 1), x.grad.permute(0, 2, 3, 1)] + [w.grad for w in ws] + [b.grad for b in bs]


def _block_gpu(x, ws, bs, gy, form):
    from tpgsr_amd import functional as Fh
    x = x.to(DEV).requires_grad_(True)
    ws = [w.to(DEV).requires_grad_(True) for w in ws]
    bs = [b.to(DEV).requires_grad_(True) for b in bs]
    y = Fh.dense_block(x, ws, bs, 0.2, 0.2, form=form)
    (y * gy.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return [t.detach().cpu() for t in [y, x.grad] + [w.grad for w in ws] + [b.grad for b in bs]]


KEYS = ["y", "dx"] + [f"dw{k}" for k in range(1, 6)] + [f"db{k}" for k in range(1, 6)]


@pytest.mark.parametrize("hw", [(5, 7), (16, 64)], ids=["5x7", "16x64"])
def test_dense_block_in_place_equals_composed(hw):
    from tpgsr_amd import kernels as K
    ins = _block_inputs(hw)
    with K.policy("x3"):
        a, b = _block_gpu(*ins, "inplace"), _block_gpu(*ins, "composed")
    for k, u, v in zip(KEYS, a, b):
        e = err(u, v)
        print(f"{hw} {k}: in place against composed {e:.2e}")
        assert tuple(u.shape) == tuple(v.shape) and e <= 1e-6, (k, e)


@pytest.mark.parametrize("form", ["inplace", "composed"])
@pytest.mark.parametrize("hw", [(5, 7), (16, 64)], ids=["5x7", "16x64"])
def test_dense_block_against_float64(hw, form):
    from tpgsr_amd import kernels as K
    ins = _block_inputs(hw)
    r64, r32 = _block_ref(*ins, torch.float64), _block_ref(*ins, torch.float32)
    with K.policy("f32"):
        got = _block_gpu(*ins, form)
    for k, g, a, b in zip(KEYS, got, r64, r32):
        e_gpu, e32 = err(g, a), err(b, a)
        bound = 4 * e32 + FLOOR
        print(f"{form} {hw} {k}: e_gpu {e_gpu:.2e}  e_ref32 {e32:.2e}  bound {bound:.2e}")
        assert tuple(g.shape) == tuple(a.shape) and e_gpu <= bound, (form, k, e_gpu, bound)


def test_default_form_and_refusals():
    from tpgsr_amd import functional as Fh
    x, ws, bs, _ = _block_inputs((5, 7))
    with pytest.raises(ValueError, match="form"):
        Fh.dense_block(x.to(DEV), [w.to(DEV) for w in ws], None, form="fused")
    with pytest.raises(ValueError, match="weight 2"):
        Fh.dense_block(x.to(DEV), [ws[0], ws[0], ws[2], ws[3], ws[4]], None)
    assert Fh.DENSE_DEFAULT_FORM in Fh.DENSE_FORMS


# ---- 1. against the fixtures (x3) ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", DEPTHS)
@pytest.mark.parametrize("scale", SCALES)
def test_rrdb_vs_reference_fixture(scale, nb, golden_dir):
    """module(x) under autograd: the SR image, every parameter gradient for the seeded upstream gradient, the 12x40 eval forward"""
    P.check_vs_fixture(P.RRDB, scale, nb, golden_dir)


@pytest.mark.parametrize("nb", DEPTHS)
@pytest.mark.parametrize("scale", SCALES)
def test_rrdb_train_step_vs_reference_trajectory(scale, nb, golden_dir):
    """two steps of the reference loop body (interfaces/super_resolution.py:409-424 with nn.L1Loss) through SRTrainStep"""
    P.check_trajectory(P.RRDB, scale, nb, golden_dir)


# ---- 2. recorded against operator by operator, capture + replay, the serial schedule, the two-term policy ---------------------------
@pytest.mark.parametrize("scale", SCALES)
def test_recorded_plan_equals_operator_by_operator_run(scale):
    P.check_recorded_equals_eager(P.RRDB, scale)


@pytest.mark.parametrize("scale", SCALES)
def test_capture_replay_equals_eager_steps(scale):
    """two replays are bitwise the eager twin's second and third step"""
    P.check_capture_replay(P.RRDB, scale)


@pytest.mark.parametrize("scale", SCALES)
def test_recorded_step_equals_serial_schedule(scale, schedule):  # noqa: F811
    """the weight-gradient launches of a dense block read windows of the in-place gradient buffer G on the side stream while the caller's
    stream goes on accumulating into the columns in front of them: the default schedule must give the bits of the SAME step replayed in
    recording order on one stream (nb 2, N 4; fresh networks record their own plans in serial mode)"""
    P.check_serial_schedule(P.RRDB, scale, schedule)


@pytest.mark.parametrize("scale,nb", [(4, 2), (2, 23)])
def test_two_term_policy_holds_the_gates(scale, nb):
    """the step's default policy x2 against x3 on the same batch and weights, with the bounds tests/test_policy_x2_gpu.py sets:
    |dPSNR| < 1e-3 dB, loss within 2e-5, gradient norm within 2e-3"""
    P.check_two_term_gates(P.RRDB, scale, nb)


# ---- 3. the prior-free pass of the evaluator --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", SCALES)
def test_evaluator_pass(scale, golden_dir):
    P.check_evaluator_pass(P.RRDB, scale, golden_dir)
