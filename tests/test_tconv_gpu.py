"""GPU: nn.ConvTranspose2d(Cin, Cout, 4, stride 2, padding 1, bias=False) on the HIP kernels (csrc/tconv4s2.hip, functional.conv_transpose2d_k4s2).

  expand / fold   pure gathers: bit-exact against an index-level restatement, guard words around every output, 16-byte aligned and
                  unaligned destinations (the vector and the scalar store paths).
  k4s2            the functional op (sub-pixel form for 64 -> 64, zero-dilated otherwise) against float64 F.conv_transpose2d: forward, data
                  gradient, weight gradient.
  narrow          the direct kernels for up to four channels: the same comparison, two runs bitwise equal, refusals before a launch.

The bound wherever a kernel is compared with float64 is the project's rule for arithmetic (tests/test_functional_ops_gpu.py, kernel_table.py):
e_gpu <= 4 * e_ref32 + 4 * 2^-24, e = max |got - ref64| / max |ref64|, e_ref32 = the error of stock float32 PyTorch on the CPU against the
same float64 reference, computed here.  Under the two-term policy x2 the bound is scaled as conftest's golden_policy scales every
forward tolerance.  Each test prints e_gpu / bound."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_functional_ops_gpu import FLOOR, _gen, err  # noqa: E402

DEV = "cuda"
F64 = torch.float64
SENTINEL = -12345.5


# ---- expand / fold ---------------------------------------------------------------------------------------------------------------------
def expand_ref(w):
    """w [Cin][Cout][4][4] -> w3 [4 Cout][Cin][3][3], index by index: channel co*4 + a*2 + b, tap (r, s) <- w[a - 2r + 3][b - 2s + 3]"""
    Cin, Cout = w.shape[:2]
    w3 = torch.zeros(Cout, 2, 2, Cin, 3, 3, dtype=w.dtype)
    for a in range(2):
        for b in range(2):
            for r in range(3):
                for s in range(3):
                    kh, kw = a - 2 * r + 3, b - 2 * s + 3
                    if 0 <= kh < 4 and 0 <= kw < 4:
                        w3[:, a, b, :, r, s] = w[:, :, kh, kw].t()
    return w3.reshape(4 * Cout, Cin, 3, 3)


def fold_ref(dw3):
    C4, Cin = dw3.shape[:2]
    Cout = C4 // 4
    v = dw3.reshape(Cout, 2, 2, Cin, 3, 3)
    dw = torch.full((Cin, Cout, 4, 4), float("nan"), dtype=dw3.dtype)
    for a in range(2):
        for b in range(2):
            for r in range(3):
                for s in range(3):
                    kh, kw = a - 2 * r + 3, b - 2 * s + 3
                    if 0 <= kh < 4 and 0 <= kw < 4:
                        dw[:, :, kh, kw] = v[:, a, b, :, r, s].t()
    assert not dw.isnan().any()      # one-to-one on the 16 taps
    return dw


def guarded(n, lead, fill=None):
    """a device buffer of n floats with `lead` guard words in front and 4 behind (lead 4: 16-byte aligned; lead 1: not)"""
    buf = torch.full((lead + n + 4,), SENTINEL, device=DEV)
    view = buf[lead:lead + n]
    if fill is not None:
        view.copy_(fill.reshape(-1))
    return buf, view


def guards_intact(buf, lead, n):
    return bool((buf[:lead] == SENTINEL).all() and (buf[lead + n:] == SENTINEL).all())


@pytest.mark.parametrize("lead", [4, 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("Cin,Cout", [(64, 64), (8, 8), (3, 5)])
def test_expand_and_fold_are_exact_gathers(Cin, Cout, lead):
    from tpgsr_amd import kernels as K
    g = _gen("tconv_expand", Cin, Cout)
    w = torch.randn(Cin, Cout, 4, 4, generator=g)
    want = expand_ref(w)
    assert int((want != 0).sum()) == 16 * Cin * Cout      # 4 of the 9 taps of each of the 4 phases
    buf, w3 = guarded(want.numel(), lead)
    assert (w3.data_ptr() % 16 == 0) == (lead == 4)
    K.tconv4s2_expand(w.to(DEV), Cin, Cout, w3)
    torch.cuda.synchronize()
    assert torch.equal(w3.cpu().reshape(want.shape), want) and guards_intact(buf, lead, want.numel())
    # fold: accumulate off (over garbage) and on (over a random dw0)
    dw3 = torch.randn(4 * Cout, Cin, 3, 3, generator=g)
    dw0 = torch.randn(Cin, Cout, 4, 4, generator=g)
    gathered = fold_ref(dw3)
    for accumulate, expect in ((False, gathered), (True, dw0 + gathered)):
        buf, dw = guarded(dw0.numel(), lead, dw0)
        K.tconv4s2_fold_grad(dw3.to(DEV), Cin, Cout, dw, accumulate=accumulate)
        torch.cuda.synchronize()
        assert torch.equal(dw.cpu().reshape(dw0.shape), expect), (accumulate, lead)
        assert guards_intact(buf, lead, dw0.numel())
    # the two are inverse on the live taps
    buf, back = guarded(w.numel(), lead)
    K.tconv4s2_fold_grad(w3, Cin, Cout, back, accumulate=False)
    torch.cuda.synchronize()
    assert torch.equal(back.cpu().reshape(w.shape), w)


# ---- the layer against float64 ---------------------------------------------------------------------------------------------------------
def make_case(tag, N, H, W, Cin, Cout):
    g = _gen("tconv_k4s2", tag, N, H, W, Cin, Cout)
    x = torch.randn(N, H, W, Cin, generator=g)
    w = torch.randn(Cin, Cout, 4, 4, generator=g) / (4 * Cin) ** 0.5      # (four taps of each input channel reach an output)
    gy = torch.randn(N, 2 * H, 2 * W, Cout, generator=g)
    return x, w, gy


def reference(x, w, gy, dtype):
    x = x.detach().clone().to(dtype).requires_grad_(True)      # (a copy: .to() of the same dtype would mark the caller's tensor)
    w = w.detach().clone().to(dtype).requires_grad_(True)
    y = F.conv_transpose2d(x.permute(0, 3, 1, 2), w, stride=2, padding=1).permute(0, 2, 3, 1)
    y.backward(gy.to(dtype))
    return dict(y=y.detach(), dx=x.grad, dw=w.grad)


def run_gpu(x, w, gy, form=None):
    """-> (results, names of the launches)"""
    from tpgsr_amd import functional as Fh, kernels as K
    names = []
    inner = K._launch

    def spy(name, *a):
        names.append(name)
        return inner(name, *a)

    xd, wd = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    K._launch = spy
    try:
        y = Fh.conv_transpose2d_k4s2(xd, wd, form)
        y.backward(gy.to(DEV))
        torch.cuda.synchronize()
    finally:
        K._launch = inner
    return dict(y=y.detach().cpu(), dx=xd.grad.cpu(), dw=wd.grad.cpu()), names


def check_against_float64(tag, got, x, w, gy, widen=1.0):
    r64, r32 = reference(x, w, gy, F64), reference(x, w, gy, torch.float32)
    worst = 0.0
    for k in ("y", "dx", "dw"):
        assert got[k].shape == r64[k].shape, (tag, k)
        e_gpu, e32 = err(got[k], r64[k]), err(r32[k], r64[k])
        bound = widen * (4 * e32 + FLOOR)
        print(f"   {tag} {k}: e_gpu {e_gpu:.2e}  e_ref32 {e32:.2e}  e_gpu / bound {e_gpu / bound:.2f}")
        worst = max(worst, e_gpu / bound)
    assert worst <= 1.0, (tag, worst)


K4S2_SHAPES = [(1, 1, 1, 64, 64), (2, 3, 5, 64, 64), (1, 1, 7, 64, 64), (1, 16, 64, 64, 64), (2, 4, 6, 8, 8)]


@pytest.mark.parametrize("shape", K4S2_SHAPES, ids=["x".join(map(str, s)) for s in K4S2_SHAPES])
def test_conv_transpose2d_k4s2_vs_float64_x3(shape):
    from tpgsr_amd import kernels as K
    x, w, gy = make_case("x3", *shape)
    with K.policy("x3"):
        got, names = run_gpu(x, w, gy)
    if shape[3:] == (64, 64):      # the sub-pixel route: expansion, pixel-shuffle convolution, fold; nothing zero-dilated
        assert names.count("tpgsr_tconv4s2_expand") == 1 and names.count("tpgsr_tconv4s2_fold_grad") == 1
        assert names.count("tpgsr_conv_fwd") == 2 and names.count("tpgsr_conv_wgrad") == 1 and names.count("tpgsr_wgrad_reduce") == 1
        assert "tpgsr_dilate2d" not in names and "tpgsr_subsample2d" not in names
    else:
        assert "tpgsr_dilate2d" in names and "tpgsr_tconv4s2_expand" not in names
    check_against_float64("x".join(map(str, shape)), got, x, w, gy)


def test_conv_transpose2d_k4s2_under_the_golden_policies(golden_policy):
    """one shape under x3 and under the two-term policy x2, the bound scaled the way conftest scales forward tolerances"""
    shape = (2, 3, 5, 64, 64)
    x, w, gy = make_case("policy", *shape)
    got, names = run_gpu(x, w, gy)
    assert names.count("tpgsr_tconv4s2_expand") == 1 and "tpgsr_dilate2d" not in names
    check_against_float64(f"{golden_policy.name} " + "x".join(map(str, shape)), got, x, w, gy, widen=golden_policy.tol(1.0))


def test_subpixel_and_zero_dilated_forms_agree():
    from tpgsr_amd import kernels as K
    shape = (2, 3, 5, 64, 64)
    x, w, gy = make_case("forms", *shape)
    with K.policy("x3"):
        sub, n_sub = run_gpu(x, w, gy, form="subpixel")
        dil, n_dil = run_gpu(x, w, gy, form="dilated")
    assert "tpgsr_dilate2d" in n_dil and "tpgsr_dilate2d" not in n_sub
    r64, r32 = reference(x, w, gy, F64), reference(x, w, gy, torch.float32)
    for k in ("y", "dx", "dw"):
        bound = 4 * err(r32[k], r64[k]) + FLOOR
        d = (sub[k].double() - dil[k].double()).abs().max().item() / r64[k].abs().max().item()
        print(f"   forms {k}: |sub - dilated| / max|ref| {d:.2e}  / bound {d / bound:.2f}")
        assert d <= bound, (k, d, bound)


# ---- the narrow kernels ----------------------------------------------------------------------------------------------------------------
SMALL_SHAPES = [(1, 1, 1, 3, 3), (2, 3, 5, 3, 3), (2, 2, 7, 4, 4), (2, 3, 5, 2, 3), (1, 16, 64, 4, 4)]


@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=["x".join(map(str, s)) for s in SMALL_SHAPES])
def test_narrow_kernels_vs_float64_and_bitwise_reproducible(shape):
    x, w, gy = make_case("small", *shape)
    got, names = run_gpu(x, w, gy)
    assert names == ["tpgsr_tconv4s2_small_fwd", "tpgsr_tconv4s2_small_bwd_data", "tpgsr_tconv4s2_small_bwd_weight", "tpgsr_reduce_partials"]
    check_against_float64("x".join(map(str, shape)), got, x, w, gy)
    again, _ = run_gpu(x, w, gy)
    for k in ("y", "dx", "dw"):
        assert torch.equal(got[k], again[k]), k


def test_narrow_kernels_write_inside_their_outputs():
    """guard words around y, dx and the partial sums at an odd shape with more than one workgroup of input positions"""
    from tpgsr_amd import kernels as K
    N, H, W, Cin, Cout = 3, 7, 19, 3, 2
    x, w, gy = make_case("guards", N, H, W, Cin, Cout)
    xd, wd, gd = x.to(DEV), w.to(DEV), gy.to(DEV)
    nblk, E = 5, Cin * Cout * 16
    by, y = guarded(gy.numel(), 4)
    bx, dx = guarded(x.numel(), 4)
    bp, part = guarded(nblk * E, 4)
    K.tconv4s2_small_fwd(xd, wd, N, H, W, Cin, Cout, y)
    K.tconv4s2_small_bwd_data(gd, wd, N, H, W, Cin, Cout, dx)
    K.tconv4s2_small_bwd_weight(xd, gd, N, H, W, Cin, Cout, part, nblk)
    dw = torch.empty(Cin, Cout, 4, 4, device=DEV)
    K.reduce_partials(part, nblk, E, dw, accumulate=False)
    torch.cuda.synchronize()
    assert guards_intact(by, 4, gy.numel()) and guards_intact(bx, 4, x.numel()) and guards_intact(bp, 4, nblk * E)
    assert not (y == SENTINEL).any() and not (dx == SENTINEL).any() and not (part == SENTINEL).any()
    r64 = reference(x, w, gy, F64)
    for k, t in (("y", y.reshape(gy.shape)), ("dx", dx.reshape(x.shape)), ("dw", dw)):
        assert err(t.cpu(), r64[k]) < 1e-5, k


def test_narrow_kernels_refuse_other_channel_counts_before_a_launch():
    from tpgsr_amd import _lib, kernels as K
    x = torch.rand(1, 2, 2, 5, device=DEV)
    w = torch.rand(5, 3, 4, 4, device=DEV)
    y = torch.full((1, 4, 4, 3), SENTINEL, device=DEV)
    with pytest.raises(ValueError, match="5 -> 3"):
        K.tconv4s2_small_fwd(x, w, 1, 2, 2, 5, 3, y)
    # the C launch functions themselves: an error code, nothing launched
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    assert lib.tpgsr_tconv4s2_small_fwd(x.data_ptr(), w.data_ptr(), 1, 2, 2, 5, 3, y.data_ptr(), s) != 0
    assert b"Cin 5" in lib.tpgsr_last_error()
    assert lib.tpgsr_tconv4s2_small_bwd_data(y.data_ptr(), w.data_ptr(), 1, 2, 2, 3, 5, x.data_ptr(), s) != 0
    assert lib.tpgsr_tconv4s2_small_bwd_weight(x.data_ptr(), y.data_ptr(), 1, 2, 2, 0, 3, w.data_ptr(), 4, s) != 0
    assert lib.tpgsr_tconv4s2_small_fwd(x.data_ptr(), w.data_ptr(), 1 << 15, 1 << 6, 1 << 6, 3, 3, y.data_ptr(), s) != 0      # 2^27 positions
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all())
