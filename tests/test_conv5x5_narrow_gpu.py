"""GPU: the direct 5x5 pad-2 convolution with optional bias to at most four output channels (csrc/conv_narrow5.hip,
functional.conv2d_narrow5x5) -- SRCNN's conv3.

Forward, data gradient, weight gradient and bias gradient against float64 F.conv2d under the project's rule for arithmetic
(tests/kernel_table.py): e_gpu <= 4 * e_ref32 + 4 * 2^-24, e = max |got - ref64| / max |ref64|, e_ref32 = the error of stock float32
PyTorch on the CPU against the same float64 reference, computed here.  The kernels are plain fp32 under every policy, so the rule applies
as it stands.  Shapes (N, H, W, Cin, Cout): every tap but the centre padding; an image smaller than the window on both axes; SRCNN's
geometry at small size with and without bias; Cin neither 32 nor 64 with Cout at its maximum (an odd number of channel groups: the data
gradient's last lane of a pixel owns one group); a row of 130 pixels at the largest Cin (an even and an odd row length both occur: the
forward's last lane of a row owns one pixel); the real row shape.  The kernels have no grid-stride loop: the grid covers every output
element, so there is no shape at which one would run twice.  Also: guard words around every output on the 16-byte and the element-wise
path, two runs bitwise equal, zero rows for workgroups behind the last pixel, accumulation onto pre-filled sinks, the two forms of
conv2d_narrow5x5 within CONV_LIMITS under x3, the policy leaving the narrow form alone, refusals before a launch."""
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_functional_ops_gpu import CONV_LIMITS, FLOOR, _gen, err  # noqa: E402

DEV = "cuda"
SENTINEL = float("nan")

# (N, H, W, Cin, Cout, bias)
CASES = [(1, 1, 1, 4, 1, True), (2, 3, 4, 32, 3, True), (2, 6, 7, 32, 3, True), (2, 6, 7, 32, 3, False), (3, 5, 9, 12, 4, True),
         (2, 3, 130, 64, 3, False), (1, 32, 128, 32, 3, True)]
IDS = ["1x1", "3x4", "6x7", "6x7_nobias", "cin12", "row130", "row_shape"]
KEYS = ("y", "dx", "dw", "db")


@functools.lru_cache(maxsize=None)
def case(shape):
    N, H, W, Cin, Cout, bias = shape
    g = _gen("conv5x5_narrow", *shape)
    x = torch.randn(N, H, W, Cin, generator=g)
    w = torch.randn(Cout, Cin, 5, 5, generator=g) / (25 * Cin) ** 0.5
    b = torch.randn(Cout, generator=g) if bias else None
    gy = torch.randn(N, H, W, Cout, generator=g)
    return x, w, b, gy


@functools.lru_cache(maxsize=None)
def reference(shape, dtype):
    x, w, b, gy = case(shape)
    x = x.detach().clone().to(dtype).requires_grad_(True)
    w = w.detach().clone().to(dtype).requires_grad_(True)
    b = None if b is None else b.detach().clone().to(dtype).requires_grad_(True)
    y = F.conv2d(x.permute(0, 3, 1, 2), w, b, padding=2).permute(0, 2, 3, 1)
    y.backward(gy.to(dtype))
    return dict(y=y.detach(), dx=x.grad, dw=w.grad, db=None if b is None else b.grad)


def run_gpu(shape, form="narrow"):
    from tpgsr_amd import functional as Fh
    x, w, b, gy = case(shape)
    x = x.to(DEV).requires_grad_(True)
    w = w.to(DEV).requires_grad_(True)
    b = None if b is None else b.to(DEV).requires_grad_(True)
    y = Fh.conv2d_narrow5x5(x, w, b, form=form)
    y.backward(gy.to(DEV))
    torch.cuda.synchronize()
    return dict(y=y.detach().cpu(), dx=x.grad.cpu(), dw=w.grad.cpu(), db=None if b is None else b.grad.cpu())


@pytest.mark.parametrize("shape", CASES, ids=IDS)
def test_narrow5_against_float64(shape):
    r64, r32 = reference(shape, torch.float64), reference(shape, torch.float32)
    a, b = run_gpu(shape), run_gpu(shape)
    for k in KEYS:
        if r64[k] is None:
            assert k == "db" and a[k] is None and not shape[5]
            continue
        e_gpu, e32 = err(a[k], r64[k]), err(r32[k], r64[k])
        bound = 4 * e32 + FLOOR
        print(f"{shape} {k}: e_gpu {e_gpu:.2e}  e_ref32 {e32:.2e}  bound {bound:.2e}")
        assert tuple(a[k].shape) == tuple(r64[k].shape) and e_gpu <= bound, (shape, k, e_gpu, bound)
        assert torch.equal(a[k], b[k]), (shape, k, "two runs differ")


def guarded(n, lead, fill=None):
    """a device buffer of n floats with `lead` NaN guard words in front and 4 behind (lead 4: 16-byte aligned; lead 1: not)"""
    buf = torch.full((lead + n + 4,), SENTINEL, device=DEV)
    view = buf[lead:lead + n]
    if fill is not None:
        view.copy_(fill.reshape(-1))
    return buf, view


def guards_intact(buf, lead, n):
    return bool(buf[:lead].isnan().all() and buf[lead + n:].isnan().all() and not buf[lead:lead + n].isnan().any())


@pytest.mark.parametrize("lead", [4, 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("shape", [(2, 6, 7, 32, 3, True), (3, 5, 9, 12, 4, True), (2, 3, 130, 64, 3, False)], ids=["6x7", "cin12", "row130"])
def test_guard_words_and_both_access_paths(shape, lead):
    """the kernels at the C ABI's level on buffers between NaN guard words: nothing outside an output is written, every output element is
    (no NaN is left inside), and the element-wise path (pointers off a 16-byte boundary) computes what the 16-byte path does, bit for bit;
    the rows of workgroups behind the last pixel are zeros"""
    from tpgsr_amd import kernels as K
    N, H, W, Cin, Cout, _ = shape
    x, w, b, gy = case(shape)
    want = run_gpu(shape)
    E, R = Cout * Cin * 25, K.narrow5_row(Cin, Cout)
    assert R == E + Cout
    _, xd = guarded(x.numel(), lead, x)
    _, wd = guarded(w.numel(), lead, w)
    _, gd = guarded(gy.numel(), lead, gy)
    bd = None if b is None else guarded(Cout, lead, b)[1]
    assert (xd.data_ptr() % 16 == 0) == (lead == 4)
    ybuf, y = guarded(N * H * W * Cout, lead)
    K.conv5x5_narrow_fwd(xd, wd, bd, N, H, W, Cin, Cout, y)
    dxbuf, dx = guarded(x.numel(), lead)
    K.conv5x5_narrow_bwd_data(gd, wd, N, H, W, Cin, Cout, dx)
    M = N * H * W
    nblk = M + 3                                             # one pixel per workgroup, three workgroups behind the last pixel
    pbuf, part = guarded(nblk * R, lead)
    K.conv5x5_narrow_bwd_weight(xd, gd, N, H, W, Cin, Cout, part, nblk)
    gbuf, grad = guarded(R, lead)
    K.reduce_partials(part, nblk, R, grad, accumulate=False)
    torch.cuda.synchronize()
    assert float(part.reshape(nblk, R)[-3:].abs().max()) == 0.0 and float(part.reshape(nblk, R)[M - 1].abs().max()) > 0.0
    assert guards_intact(ybuf, lead, y.numel()) and guards_intact(dxbuf, lead, dx.numel())
    assert guards_intact(pbuf, lead, part.numel()) and guards_intact(gbuf, lead, R)
    assert torch.equal(y.cpu().reshape(want["y"].shape), want["y"])
    assert torch.equal(dx.cpu().reshape(want["dx"].shape), want["dx"])
    # the weight gradient over another split of the pixels: the same sums in another association, so the arithmetic rule, not bits
    r64, r32 = reference(shape, torch.float64), reference(shape, torch.float32)
    for k, got in (("dw", grad[:E].cpu().reshape(w.shape)),) + ((("db", grad[E:].cpu()),) if b is not None else ()):
        assert err(got, r64[k]) <= 4 * err(r32[k], r64[k]) + FLOOR, k
    # the op's own split, on these buffers: bit for bit the op's result on either access path
    own = K.narrow5_wgrad_blocks(N, H, W)
    pbuf2, part2 = guarded(own * R, lead)
    K.conv5x5_narrow_bwd_weight(xd, gd, N, H, W, Cin, Cout, part2, own)
    gbuf2, grad2 = guarded(R, lead)
    K.reduce_partials(part2, own, R, grad2, accumulate=False)
    torch.cuda.synchronize()
    assert guards_intact(pbuf2, lead, part2.numel()) and guards_intact(gbuf2, lead, R)
    assert torch.equal(grad2[:E].cpu().reshape(w.shape), want["dw"])
    if b is not None:
        assert torch.equal(grad2[E:].cpu(), want["db"])


def test_gradients_accumulate_onto_prefilled_sinks():
    from tpgsr_amd import functional as Fh
    shape = (2, 6, 7, 32, 3, True)
    x, w, b, gy = case(shape)
    plain = run_gpu(shape)
    g = _gen("conv5x5_narrow_sink")
    fill_w, fill_b = torch.randn(w.shape, generator=g), torch.randn(b.shape, generator=g)
    wd, bd = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    sink_w, sink_b = fill_w.to(DEV).clone(), fill_b.to(DEV).clone()
    with Fh.grad_sinks({wd.data_ptr(): sink_w, bd.data_ptr(): sink_b}):
        y = Fh.conv2d_narrow5x5(x.to(DEV).requires_grad_(True), wd, bd, form="narrow")
        y.backward(gy.to(DEV))
        torch.cuda.synchronize()
    assert wd.grad is None and bd.grad is None
    assert torch.equal(sink_w.cpu(), fill_w + plain["dw"])             # one fp32 addition per element, on either side
    assert torch.equal(sink_b.cpu(), fill_b + plain["db"])


@pytest.mark.parametrize("shape", [(2, 6, 7, 32, 3, True), (1, 32, 128, 32, 3, True), (3, 5, 9, 12, 4, True)], ids=["6x7", "row_shape", "cin12"])
def test_the_two_forms_agree_under_x3(shape):
    from tpgsr_amd import kernels as K
    with K.policy("x3"):
        a, b = run_gpu(shape, "narrow"), run_gpu(shape, "matrix")
    for k in KEYS:
        e = err(a[k], b[k])
        bound = CONV_LIMITS["x3"][1 if k in ("dw", "db") else 0]
        print(f"{shape} {k}: narrow against matrix {e:.2e} (bound {bound:.0e})")
        assert e <= bound, (shape, k, e)


def test_policy_does_not_touch_the_narrow_form():
    from tpgsr_amd import kernels as K
    shape = (3, 5, 9, 12, 4, True)
    with K.policy("x3"):
        a = run_gpu(shape)
    with K.policy("x2"):
        b = run_gpu(shape)
    with K.policy("f32"):
        c = run_gpu(shape)
    for k in KEYS:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k


def test_refusals_come_before_a_launch():
    from tpgsr_amd import _lib, functional as Fh, kernels as K
    x = torch.zeros(1, 4, 4, 8, device=DEV)
    w = torch.zeros(3, 8, 5, 5, device=DEV)
    with pytest.raises(ValueError, match="form"):
        Fh.conv2d_narrow5x5(x, w, form="direct")
    with pytest.raises(ValueError, match="weight"):
        Fh.conv2d_narrow5x5(x, torch.zeros(5, 8, 5, 5, device=DEV))
    with pytest.raises(ValueError, match="weight"):
        Fh.conv2d_narrow5x5(x, torch.zeros(3, 8, 3, 3, device=DEV))
    with pytest.raises(ValueError, match="input"):
        Fh.conv2d_narrow5x5(x, torch.zeros(3, 12, 5, 5, device=DEV))
    with pytest.raises(ValueError, match="bias"):
        Fh.conv2d_narrow5x5(x, w, torch.zeros(4, device=DEV))
    with pytest.raises(ValueError, match="multiple of 4"):
        Fh.conv2d_narrow5x5(torch.zeros(1, 4, 4, 6, device=DEV), torch.zeros(3, 6, 5, 5, device=DEV), form="narrow")
    with pytest.raises(ValueError, match="multiple of 4"):
        Fh.conv2d_narrow5x5(torch.zeros(1, 2, 2, 68, device=DEV), torch.zeros(3, 68, 5, 5, device=DEV), form="narrow")
    y = torch.zeros(1, 4, 4, 3, device=DEV)
    with pytest.raises(ValueError, match="sizes"):
        K.conv5x5_narrow_fwd(x, w, None, 1, 4, 5, 8, 3, y)
    with pytest.raises(ValueError, match="sizes"):
        K.conv5x5_narrow_fwd(x, w, torch.zeros(2, device=DEV), 1, 4, 4, 8, 3, y)
    with pytest.raises(ValueError, match="partial"):
        K.conv5x5_narrow_bwd_weight(x, y, 1, 4, 4, 8, 3, torch.zeros(10, device=DEV), 2)
    # the C entry points refuse on their own
    lib = _lib.load()
    X, Y = x.data_ptr(), y.data_ptr()
    for geom in ((1, 4, 4, 6, 3), (1, 4, 4, 68, 3), (1, 4, 4, 8, 5), (1 << 9, 1 << 9, 1 << 9, 8, 3)):
        assert lib.tpgsr_conv5x5_narrow_fwd(X, X, None, *geom, Y, None) == -1
        assert lib.tpgsr_conv5x5_narrow_bwd_data(X, X, *geom, Y, None) == -1
        assert lib.tpgsr_conv5x5_narrow_bwd_weight(X, X, *geom, Y, 1, None) == -1
    assert lib.tpgsr_conv5x5_narrow_fwd(None, X, None, 1, 4, 4, 8, 3, Y, None) == -1
    assert lib.tpgsr_conv5x5_narrow_bwd_data(X, None, 1, 4, 4, 8, 3, Y, None) == -1
    assert lib.tpgsr_conv5x5_narrow_bwd_weight(X, X, 1, 4, 4, 8, 3, None, 1, None) == -1
    assert lib.tpgsr_conv5x5_narrow_bwd_weight(X, X, 1, 4, 4, 8, 3, Y, 0, None) == -1
    torch.cuda.synchronize()
    assert y.abs().sum().item() == 0
