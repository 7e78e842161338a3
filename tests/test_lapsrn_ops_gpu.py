"""GPU: the element-wise kernels `--arch lapsrn` adds -- tpgsr_leaky_relu_fwd / _bwd (bit-exact against stock PyTorch) and
tpgsr_charbonnier_loss_fwd / _bwd (L1_Charbonnier_loss: a SUM of sqrt(d^2 + eps)) against float64 with the project's rule for arithmetic,
e_gpu <= 4 * e_ref32 + 4 * 2^-24 (tests/kernel_table.py: for a scalar, e_ref32 is the worst float32-CPU error over SCALAR_SEEDS seeds at the
case's shape).  Each comparison prints e_gpu / bound."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_table import SCALAR_SEEDS  # noqa: E402
from test_functional_ops_gpu import FLOOR, _gen, err  # noqa: E402

DEV = "cuda"
F64 = torch.float64
EPS = 1e-6


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- LeakyReLU ---------------------------------------------------------------------------------------------------------------------------
def leaky_inputs(n):
    g = _gen("leaky", n)
    x = torch.randn(n, generator=g)
    dy = torch.randn(n, generator=g)
    tiny = torch.finfo(torch.float32).tiny
    special = torch.tensor([0.0, -0.0, tiny / 4, -tiny / 4, tiny, -tiny, 1e-45, -1e-45, 3.0, -3.0, float("inf"), -float("inf")])
    k = min(n, special.numel())
    x[:k] = special[:k]
    dy[k:2 * k] = special[:max(0, min(k, n - k))]      # (special upstream gradients on ordinary x)
    return x, dy


@pytest.mark.parametrize("n", [1, 3, 4099, 2 * 5 * 7 * 64])
@pytest.mark.parametrize("slope", [0.2, 0.01])
def test_leaky_relu_is_bit_exact(n, slope):
    from tpgsr_amd import functional as Fh
    x, dy = leaky_inputs(n)
    xr = x.clone().requires_grad_(True)
    yr = F.leaky_relu(xr, slope)
    yr.backward(dy)
    xd = x.to(DEV).requires_grad_(True)
    y = Fh.leaky_relu(xd, slope)
    y.backward(dy.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(bits(y.detach().cpu()), bits(yr.detach())), "forward"      # bit patterns: the sign of zero and denormals included
    assert torch.equal(bits(xd.grad.cpu()), bits(xr.grad)), "backward"
    if n > 1:      # x = +0 and x = -0: the derivative at x <= 0 is the slope
        assert torch.equal(xd.grad[:2].cpu(), dy[:2] * slope)


def test_leaky_relu_unaligned_views_and_guards():
    """the scalar path (a destination that is not 16-byte aligned) and the words around the output"""
    from tpgsr_amd import kernels as K
    n = 1031
    x, dy = leaky_inputs(n)
    buf = torch.full((n + 9,), -7.0, device=DEV)
    out = buf[5:5 + n]
    assert out.data_ptr() % 16 != 0
    K.leaky_relu_fwd(x.to(DEV), n, 0.2, out)
    torch.cuda.synchronize()
    assert torch.equal(bits(out.cpu()), bits(F.leaky_relu(x, 0.2))) and bool((buf[:5] == -7.0).all() and (buf[5 + n:] == -7.0).all())
    K.leaky_relu_bwd(x.to(DEV), dy.to(DEV), n, 0.2, out)
    torch.cuda.synchronize()
    want = torch.where(x > 0, dy, dy * 0.2)
    assert torch.equal(bits(out.cpu()), bits(want)) and bool((buf[:5] == -7.0).all() and (buf[5 + n:] == -7.0).all())


# ---- Charbonnier -------------------------------------------------------------------------------------------------------------------------
def charb_inputs(n, seed):
    g = _gen("charbonnier", n, seed)
    out, tgt = torch.rand(n, generator=g), torch.rand(n, generator=g)
    if n >= 7:                        # planted: d = 0 (value sqrt(eps), gradient 0) and |d| = 2
        tgt[2] = out[2]
        out[4], tgt[4] = 1.5, -0.5
        out[5], tgt[5] = -1.0, 1.0
    return out, tgt


def charb_ref(out, tgt, w, dtype):
    o = out.to(dtype).requires_grad_(True)
    d = o - tgt.to(dtype)
    loss = torch.sqrt(d * d + EPS).sum() * w
    loss.backward()
    return loss.detach(), o.grad


def scalar_e32(n, w):
    """one scalar's float32 error is a lottery: the worst over the seeds at this shape"""
    return max(err(charb_ref(*charb_inputs(n, seed), w, torch.float32)[0], charb_ref(*charb_inputs(n, seed), w, F64)[0]) for seed in range(SCALAR_SEEDS))


def charb_gpu(out, tgt, w, nblk):
    from tpgsr_amd import kernels as K
    o, t = out.to(DEV), tgt.to(DEV)
    n = o.numel()
    part = torch.full((nblk, 2), float("nan"), device=DEV)
    loss = torch.zeros((), device=DEV)
    dl = torch.full((1,), 1.0, device=DEV)
    dout = torch.full((n,), float("nan"), device=DEV)
    K.charbonnier_loss_fwd(o, t, n, EPS, part, nblk)
    K.image_loss_finalize(part, nblk, 1, 0, w, 0.0, loss)      # count 1: a sum
    K.charbonnier_loss_bwd(o, t, dl, n, EPS, w, dout)
    torch.cuda.synchronize()
    assert bool((part[:, 1] == 0).all())
    return loss.cpu(), dout.cpu()


@pytest.mark.parametrize("n,nblk", [(1, 1), (7, 3), (4096, 64), (3 * 64 * 256, 1024)])
def test_charbonnier_vs_float64(n, nblk):
    w = 100.0
    out, tgt = charb_inputs(n, 0)
    l64, g64 = charb_ref(out, tgt, w, F64)
    l32, g32 = charb_ref(out, tgt, w, torch.float32)
    e32_scalar = scalar_e32(n, w)
    loss, dout = charb_gpu(out, tgt, w, nblk)
    for k, got, ref, e32 in (("value", loss, l64, e32_scalar), ("gradient", dout, g64, err(g32, g64))):
        e_gpu, bound = err(got, ref), 4 * e32 + FLOOR
        print(f"   charbonnier n {n} {k}: e_gpu {e_gpu:.2e}  e_ref32 {e32:.2e}  e_gpu / bound {e_gpu / bound:.2f}")
        assert e_gpu <= bound, (k, e_gpu, bound)
    if n >= 7:
        assert dout[2].item() == 0.0                                                 # d = 0: gradient 0
        for i, sgn in ((4, 1.0), (5, -1.0)):                                         # |d| = 2
            assert abs(dout[i].item() - sgn * w * 2.0 / (4.0 + EPS) ** 0.5) <= 2.0 ** -22 * w
    # two runs bitwise equal
    loss2, dout2 = charb_gpu(out, tgt, w, nblk)
    assert torch.equal(bits(loss.reshape(1)), bits(loss2.reshape(1))) and torch.equal(bits(dout), bits(dout2))


def test_charbonnier_planted_single_elements():
    one = torch.tensor([0.25])
    loss, dout = charb_gpu(one, one.clone(), 1.0, 1)              # d = 0: sqrt(eps), gradient 0
    assert abs(loss.item() - EPS ** 0.5) <= 2.0 ** -23 * EPS ** 0.5 and dout.item() == 0.0
    loss, dout = charb_gpu(torch.tensor([1.0]), torch.tensor([-1.0]), 1.0, 1)      # d = 2
    assert abs(loss.item() - (4.0 + EPS) ** 0.5) <= 2.0 ** -23 * 2.0 and abs(dout.item() - 2.0 / (4.0 + EPS) ** 0.5) <= 2.0 ** -23


def test_charbonnier_is_a_sum_not_a_mean():
    """doubling n with the same data doubles the value; the module computes the same sum and differentiates it"""
    from tpgsr_amd.model.lapsrn import L1_Charbonnier_loss
    out, tgt = charb_inputs(4096, 1)
    l1, _ = charb_gpu(out, tgt, 1.0, 64)
    l2, _ = charb_gpu(torch.cat([out, out]), torch.cat([tgt, tgt]), 1.0, 64)
    assert abs(l2.item() - 2.0 * l1.item()) <= FLOOR * l2.item()
    assert l1.item() > 0.2 * 4096 * 0.3                              # (a mean would be below 1)
    x = out.reshape(2, 4, 16, 32).to(DEV).requires_grad_(True)
    lm = L1_Charbonnier_loss()(x, tgt.reshape(2, 4, 16, 32).to(DEV))
    (lm * 3.0).backward()
    torch.cuda.synchronize()
    l64, g64 = charb_ref(out, tgt, 3.0, F64)
    _, g32 = charb_ref(out, tgt, 3.0, torch.float32)
    assert err(lm.detach().cpu().double() * 3.0, l64) <= 4 * scalar_e32(4096, 3.0) + FLOOR
    assert err(x.grad.cpu().reshape(-1), g64) <= 4 * err(g32, g64) + FLOOR
