"""GPU: `--arch edsr` (EDSR x2 / x4, nn.L1Loss) -- functional.res_block in both forms, the module operator by operator and through
`SRTrainStep` + engine_functional.PlainSREngine against fixtures generated from the reference's own module
(tests/golden/make_golden_edsr.py); FusedAdam over the frozen MeanShift tensors; recorded plans against the operator-by-operator run on
fresh inputs, hipGraph capture, the recorded step under the serial schedule (the side-stream reads of res_scale * dy and dz), the two-term
policy, batch independence, the prior-free evaluator pass.

Bounds (the numbers live in BOUNDS of tests/plain_arch_common.py, read through the `EDSR` entry of its Arch table; the network-level
bodies are there too): forward images 1e-4 (of max(1, |y| max)), every parameter-gradient norm 5e-3 (check_param_grads), trajectory: loss 3e-4, clip norm 3e-3, second loss 2e-2; recorded against operator by operator: SR
bitwise, gradients 1e-6; x2 against x3: |dPSNR| < 1e-3 dB, loss 2e-5, clip norm 2e-3.  The evaluator: SR 1e-4, |dPSNR| < 1e-5 dB and
dSSIM < 1e-7 against the float64 restatement, identical strings.  res_block: the fused form against the composed one within 1e-6 (of the
composed result's largest magnitude) under the default policy x3; both against float64 autograd under the `arith` rule of
tests/kernel_table.py (e_gpu <= 4 * e_ref32 + 4 * 2^-24) under policy f32, where the fused form's data gradient has no activation epilogue
and tpgsr_act_bwd runs behind it.  The block's inputs come from the first seed of BLOCK_SEEDS whose float64 pre-activations all keep
|conv1(x)| >= KINK_MARGIN: an element within float32 rounding of the ReLU's kink has derivative 0 in one arithmetic and 1 in another, and
no bound on arithmetic covers that (the pattern of POOL_SEEDS in tests/test_functional_ops_gpu.py).  One image alone against its row of a
batch: 1e-5 of max(1, |y| max) -- the convolution launches of a batch of one may split their contraction (fewer tiles than compute
units), which re-associates float32 sums of seven layers at 2^-24 each; leakage between images would be of order 1."""
import functools

import pytest
import torch
import torch.nn.functional as F

import plain_arch_common as P
from kernel_table import FLOOR, _gen, err
from make_golden_edsr import FROZEN, SEEDS      # (seeds only; the reference is not imported here)
from oracle import tpgsr_oracle as O
from plain_arch_common import schedule  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

DEV = "cuda"
SCALES = [2, 4]
DEPTHS = [2, 32]
CHANNELS = P.EDSR.channels
FORMS = ["fused", "composed"]      # the residual blocks' form (EDSR.set_form): the network-level tests run both, whichever is the default


def load(scale, nb, wseed=None, form=None):
    return P.load(P.EDSR, scale, nb, wseed, form, dev=DEV)


def make_step(net, precision="x3"):
    return P.make_step(P.EDSR, net, precision)


# ---- 0. functional.res_block ---------------------------------------------------------------------------------------------------------
C = 256
RES_SCALE = 0.1
BLOCK_SEEDS = tuple(range(16))
KINK_MARGIN = 2e-6      # ~10x the float32 accumulation error of a 2304-term sum of products of magnitude 0.02


@functools.lru_cache(maxsize=None)
def _block_inputs(hw):
    for seed in BLOCK_SEEDS:
        g = _gen("res_block", hw, seed)
        x = torch.randn(2, hw[0], hw[1], C, generator=g)
        w1, w2 = [torch.randn(C, C, 3, 3, generator=g) / (9 * C) ** 0.5 for _ in range(2)]
        gy = torch.randn(2, hw[0], hw[1], C, generator=g)
        pre = F.conv2d(x.double().permute(0, 3, 1, 2), w1.double(), padding=1)
        if float(pre.abs().min()) >= KINK_MARGIN:
            print(f"res_block {hw}: seed {seed}, min |conv1(x)| {float(pre.abs().min()):.2e}")
            return x, w1, w2, gy
    raise RuntimeError("no seed keeps the pre-activations off the ReLU's kink")


@functools.lru_cache(maxsize=None)
def _block_ref(hw, dtype):
    """stock PyTorch autograd in `dtype` (NHWC in, NHWC out): y, dx, dw1, dw2"""
    x, w1, w2, gy = _block_inputs(hw)
    x = x.to(dtype).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    w1, w2 = [w.detach().clone().to(dtype).requires_grad_(True) for w in (w1, w2)]
    y = F.conv2d(F.relu(F.conv2d(x, w1, padding=1)), w2, padding=1) * torch.tensor(RES_SCALE, dtype=torch.float32).to(dtype) + x
    (y * gy.to(dtype).permute(0, 3, 1, 2)).sum().backward()
    return [y.detach().permute(0, 2, 3, 1), x.grad.permute(0, 2, 3, 1), w1.grad, w2.grad]


def _block_gpu(hw, form):
    from tpgsr_amd import functional as Fh
    x, w1, w2, gy = _block_inputs(hw)
    x = x.to(DEV).requires_grad_(True)
    w1, w2 = [w.to(DEV).requires_grad_(True) for w in (w1, w2)]
    y = Fh.res_block(x, w1, w2, RES_SCALE, form=form)
    (y * gy.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return [t.detach().cpu() for t in (y, x.grad, w1.grad, w2.grad)]


KEYS = ["y", "dx", "dw1", "dw2"]
HWS = [(5, 7), (16, 64)]
HW_IDS = ["5x7", "16x64"]


@pytest.mark.parametrize("hw", HWS, ids=HW_IDS)
def test_res_block_fused_equals_composed(hw):
    from tpgsr_amd import kernels as K
    with K.policy("x3"):
        a, b = _block_gpu(hw, "fused"), _block_gpu(hw, "composed")
    for k, u, v in zip(KEYS, a, b):
        e = err(u, v)
        print(f"{hw} {k}: fused against composed {e:.2e}")
        assert tuple(u.shape) == tuple(v.shape) and e <= 1e-6, (k, e)


@pytest.mark.parametrize("form", ["fused", "composed"])
@pytest.mark.parametrize("hw", HWS, ids=HW_IDS)
def test_res_block_against_float64(hw, form):
    from tpgsr_amd import kernels as K
    r64, r32 = _block_ref(hw, torch.float64), _block_ref(hw, torch.float32)
    with K.policy("f32"):
        got = _block_gpu(hw, form)
    for k, g, a, b in zip(KEYS, got, r64, r32):
        e_gpu, e32 = err(g, a), err(b, a)
        bound = 4 * e32 + FLOOR
        print(f"{form} {hw} {k}: e_gpu {e_gpu:.2e}  e_ref32 {e32:.2e}  bound {bound:.2e}")
        assert tuple(g.shape) == tuple(a.shape) and e_gpu <= bound, (form, k, e_gpu, bound)


def test_res_block_refusals_and_defaults():
    from tpgsr_amd import functional as Fh
    x = torch.zeros(1, 5, 7, 8, device=DEV)
    w = torch.zeros(8, 8, 3, 3, device=DEV)
    with pytest.raises(ValueError, match="form"):
        Fh.res_block(x, w, w, form="inplace")
    with pytest.raises(ValueError, match="channels"):
        Fh.res_block(x, torch.zeros(12, 12, 3, 3, device=DEV), w)
    with pytest.raises(ValueError, match="3x3"):
        Fh.res_block(x, w, torch.zeros(8, 8, 1, 1, device=DEV))
    with pytest.raises(ValueError, match="multiple of 4"):
        Fh.res_block(torch.zeros(1, 5, 7, 6, device=DEV), torch.zeros(6, 6, 3, 3, device=DEV), torch.zeros(6, 6, 3, 3, device=DEV), form="fused")
    assert Fh.RES_DEFAULT_FORM in Fh.RES_FORMS and Fh.NARROW_DEFAULT_FORM in Fh.NARROW_FORMS


# ---- 1. against the fixtures (x3) ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nb", DEPTHS)
@pytest.mark.parametrize("scale", SCALES)
def test_edsr_vs_reference_fixture(scale, nb, form, golden_dir):
    """module(x) under autograd: the SR image, every parameter gradient for the seeded upstream gradient, the 12x40 eval forward"""
    net = P.check_vs_fixture(P.EDSR, scale, nb, golden_dir, form)
    P_ = dict(net.named_parameters())
    for k in FROZEN:                                   # no gradient is ever computed for a frozen tensor
        assert P_[k].grad is None or float(P_[k].grad.abs().max()) == 0.0, k
    assert len([k for k in P_ if k not in FROZEN]) == len(P_) - 4


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nb", DEPTHS)
@pytest.mark.parametrize("scale", SCALES)
def test_edsr_train_step_vs_reference_trajectory(scale, nb, form, golden_dir):
    """two steps of the reference loop body (interfaces/super_resolution.py:409-424 with nn.L1Loss, torch.optim.Adam over
    model.parameters()) through SRTrainStep: FusedAdam walks the whole arena and leaves the four MeanShift tensors bit for bit"""
    net, _ = P.check_trajectory(P.EDSR, scale, nb, golden_dir, form)
    for k in FROZEN:                                      # ... and their slices of the gradient arena were never written
        assert float(dict(net.named_parameters())[k].grad.abs().max()) == 0.0, k


def test_fused_adam_still_refuses_an_undeclared_frozen_parameter():
    net = load(2, 2).train()
    net.conv_mid.weight.requires_grad = False
    with pytest.raises(NotImplementedError, match="conv_mid.weight"):
        make_step(net)


# ---- 2. recorded against operator by operator, capture + replay, the serial schedule, the two-term policy ---------------------------
NB_SMALL = P.EDSR.nb_small


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("scale", SCALES)
def test_recorded_plan_equals_operator_by_operator_run(scale, form):
    P.check_recorded_equals_eager(P.EDSR, scale, form)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("scale", SCALES)
def test_capture_replay_equals_eager_steps(scale, form):
    """two replays are bitwise the eager twin's second and third step"""
    P.check_capture_replay(P.EDSR, scale, form)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("scale", SCALES)
def test_recorded_step_equals_serial_schedule(scale, form, schedule):  # noqa: F811
    """the weight-gradient launches of a residual block read res_scale * dy and dz on the side stream while the caller's stream moves on,
    conv_output's partial sums are reduced into the arena there: the default schedule must give the bits of the SAME step replayed in
    recording order on one stream (depth 2, N 4; fresh networks record their own plans in serial mode)"""
    P.check_serial_schedule(P.EDSR, scale, schedule, form)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("scale,nb", [(4, 2), (2, 32)])
def test_two_term_policy_holds_the_gates(scale, nb, form):
    """the step's default policy x2 against x3 on the same batch and weights, with the bounds tests/test_policy_x2_gpu.py sets:
    |dPSNR| < 1e-3 dB, loss within 2e-5, gradient norm within 2e-3"""
    P.check_two_term_gates(P.EDSR, scale, nb, form)


@pytest.mark.parametrize("scale", SCALES)
def test_one_image_alone_equals_its_row_of_the_batch(scale):
    from tpgsr_amd import kernels as K
    x = O.synthetic_batch(3, SEEDS[(NB_SMALL, scale)][0], scale=scale)[0][:, :CHANNELS].contiguous().to(DEV)
    net = load(scale, NB_SMALL).eval()
    with K.policy("x3"), torch.no_grad():
        yb = net(x)
        for j in range(3):
            yj = net(x[j:j + 1].contiguous())
            e = float((yj[0] - yb[j]).abs().max())
            print(f"x{scale} image {j}: alone against row {j} of the batch {e:.2e} (|y| max {float(yb.abs().max()):.2f})")
            assert e <= 1e-5 * max(1.0, float(yb.abs().max())), (j, e)


# ---- 3. the prior-free pass of the evaluator --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", SCALES)
def test_evaluator_pass(scale, golden_dir):
    P.check_evaluator_pass(P.EDSR, scale, golden_dir)
