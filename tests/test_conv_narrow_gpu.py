"""GPU: the direct 3x3 pad-1 convolution to at most four output channels (csrc/conv_narrow.hip, functional.conv2d_narrow) -- EDSR's
conv_output.

Forward, data gradient and weight gradient against float64 F.conv2d under the project's rule for arithmetic (tests/kernel_table.py):
e_gpu <= 4 * e_ref32 + 4 * 2^-24, e = max |got - ref64| / max |ref64|, e_ref32 = the error of stock float32 PyTorch on the CPU against the
same float64 reference, computed here.  The kernels are plain fp32 under every policy, so the rule applies as it stands.  Shapes
(N, H, W, Cin, Cout): every tap but the centre padding; rows shorter than a wave with the image boundary inside a run; Cin not a multiple
of 64 (lanes without channels); a row longer than one run; the real row shape; and one shape from the kernels' own constants at which the
grid-stride loop of the forward / data-gradient kernels runs twice.  Also: guard words around every output on the 16-byte and the
element-wise path, two runs bitwise equal, accumulation onto a pre-filled sink, the two forms of conv2d_narrow within CONV_LIMITS under
x3, refusals before a launch."""
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


def _stride_twice_shape():
    """rows of three pixels are one run each: one run more than a full grid of NARROW_GRID_CAP workgroups x NARROW_WAVES runs covers"""
    from tpgsr_amd import kernels as K
    H = K.NARROW_GRID_CAP * K.NARROW_WAVES // 2 + 4
    assert K.narrow_runs(2, H, 3) > K.NARROW_GRID_CAP * K.NARROW_WAVES
    return (2, H, 3, 4, 3)


SHAPES = [(1, 1, 1, 8, 1), (2, 5, 7, 256, 3), (3, 4, 9, 12, 4), (2, 3, 130, 64, 3), (1, 32, 128, 256, 3), "stride_twice"]
IDS = ["1x1", "5x7", "cin12", "row130", "row_shape", "stride_twice"]


def _shape(s):
    return _stride_twice_shape() if s == "stride_twice" else s


@functools.lru_cache(maxsize=None)
def case(shape):
    N, H, W, Cin, Cout = shape
    g = _gen("conv_narrow", *shape)
    x = torch.randn(N, H, W, Cin, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5
    gy = torch.randn(N, H, W, Cout, generator=g)
    return x, w, gy


@functools.lru_cache(maxsize=None)
def reference(shape, dtype):
    x, w, gy = case(shape)
    x = x.detach().clone().to(dtype).requires_grad_(True)
    w = w.detach().clone().to(dtype).requires_grad_(True)
    y = F.conv2d(x.permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1)
    y.backward(gy.to(dtype))
    return dict(y=y.detach(), dx=x.grad, dw=w.grad)


def run_gpu(shape, form="narrow"):
    from tpgsr_amd import functional as Fh
    x, w, gy = case(shape)
    x = x.to(DEV).requires_grad_(True)
    w = w.to(DEV).requires_grad_(True)
    y = Fh.conv2d_narrow(x, w, form=form)
    y.backward(gy.to(DEV))
    torch.cuda.synchronize()
    return dict(y=y.detach().cpu(), dx=x.grad.cpu(), dw=w.grad.cpu())


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_narrow_against_float64(shape):
    shape = _shape(shape)
    r64, r32 = reference(shape, torch.float64), reference(shape, torch.float32)
    a, b = run_gpu(shape), run_gpu(shape)
    for k in ("y", "dx", "dw"):
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
@pytest.mark.parametrize("shape", [(2, 5, 7, 256, 3), (3, 4, 9, 12, 4), (2, 3, 130, 64, 3)], ids=["5x7", "cin12", "row130"])
def test_guard_words_and_both_access_paths(shape, lead):
    """the kernels at the C ABI's level on buffers between NaN guard words: nothing outside an output is written, every output element is
    (no NaN is left inside), and the element-wise path (pointers off a 16-byte boundary) computes what the 16-byte path does, bit for bit"""
    from tpgsr_amd import kernels as K
    N, H, W, Cin, Cout = shape
    x, w, gy = case(shape)
    want = run_gpu(shape)
    E = Cout * Cin * 9
    _, xd = guarded(x.numel(), lead, x)
    _, wd = guarded(w.numel(), lead, w)
    _, gd = guarded(gy.numel(), lead, gy)
    assert (xd.data_ptr() % 16 == 0) == (lead == 4)
    ybuf, y = guarded(N * H * W * Cout, lead)
    K.conv3x3_narrow_fwd(xd, wd, N, H, W, Cin, Cout, y)
    dxbuf, dx = guarded(x.numel(), lead)
    K.conv3x3_narrow_bwd_data(gd, wd, N, H, W, Cin, Cout, dx)
    nblk = K.narrow_wgrad_blocks(N, H, W) + 3                 # (three workgroups behind the last run: their rows are zeros)
    pbuf, part = guarded(nblk * E, lead)
    K.conv3x3_narrow_bwd_weight(xd, gd, N, H, W, Cin, Cout, part, nblk)
    dwbuf, dw = guarded(E, lead)
    K.reduce_partials(part, nblk, E, dw, accumulate=False)
    torch.cuda.synchronize()
    assert guards_intact(ybuf, lead, y.numel()) and guards_intact(dxbuf, lead, dx.numel())
    assert guards_intact(pbuf, lead, part.numel()) and guards_intact(dwbuf, lead, E)
    assert torch.equal(y.cpu().reshape(want["y"].shape), want["y"])
    assert torch.equal(dx.cpu().reshape(want["dx"].shape), want["dx"])
    assert float(part.reshape(nblk, E)[-3:].abs().max()) == 0.0
    # (the op's own launch runs narrow_wgrad_blocks workgroups: the same ranges of pixels, so the same partial sums)
    assert torch.equal(dw.cpu().reshape(want["dw"].shape), want["dw"])


def test_weight_gradient_accumulates_onto_a_prefilled_sink():
    from tpgsr_amd import functional as Fh
    shape = (2, 5, 7, 256, 3)
    x, w, gy = case(shape)
    plain = run_gpu(shape)["dw"]
    g = _gen("conv_narrow_sink")
    fill = torch.randn(w.shape, generator=g)
    wd = w.to(DEV).requires_grad_(True)
    sink = fill.to(DEV).clone()
    with Fh.grad_sinks({wd.data_ptr(): sink}):
        y = Fh.conv2d_narrow(x.to(DEV).requires_grad_(True), wd, form="narrow")
        y.backward(gy.to(DEV))
        torch.cuda.synchronize()
    assert wd.grad is None
    assert torch.equal(sink.cpu(), fill + plain)             # one fp32 addition per element, on either side


@pytest.mark.parametrize("shape", [(2, 5, 7, 256, 3), (1, 32, 128, 256, 3), (3, 4, 9, 12, 4)], ids=["5x7", "row_shape", "cin12"])
def test_the_two_forms_agree_under_x3(shape):
    from tpgsr_amd import kernels as K
    with K.policy("x3"):
        a, b = run_gpu(shape, "narrow"), run_gpu(shape, "matrix")
    for k in ("y", "dx", "dw"):
        e = err(a[k], b[k])
        bound = CONV_LIMITS["x3"][1 if k == "dw" else 0]
        print(f"{shape} {k}: narrow against matrix {e:.2e} (bound {bound:.0e})")
        assert e <= bound, (shape, k, e)


def test_policy_does_not_touch_the_narrow_form():
    from tpgsr_amd import kernels as K
    shape = (3, 4, 9, 12, 4)
    with K.policy("x3"):
        a = run_gpu(shape)
    with K.policy("x2"):
        b = run_gpu(shape)
    with K.policy("f32"):
        c = run_gpu(shape)
    for k in ("y", "dx", "dw"):
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k


def test_refusals_come_before_a_launch():
    from tpgsr_amd import _lib, functional as Fh, kernels as K
    x = torch.zeros(1, 4, 4, 8, device=DEV)
    with pytest.raises(ValueError, match="form"):
        Fh.conv2d_narrow(x, torch.zeros(3, 8, 3, 3, device=DEV), form="direct")
    with pytest.raises(ValueError, match="weight"):
        Fh.conv2d_narrow(x, torch.zeros(5, 8, 3, 3, device=DEV))
    with pytest.raises(ValueError, match="weight"):
        Fh.conv2d_narrow(x, torch.zeros(3, 8, 1, 1, device=DEV))
    with pytest.raises(ValueError, match="input"):
        Fh.conv2d_narrow(x, torch.zeros(3, 12, 3, 3, device=DEV))
    with pytest.raises(ValueError, match="multiple of 4"):
        Fh.conv2d_narrow(torch.zeros(1, 4, 4, 6, device=DEV), torch.zeros(3, 6, 3, 3, device=DEV), form="narrow")
    with pytest.raises(ValueError, match="multiple of 4"):
        Fh.conv2d_narrow(torch.zeros(1, 2, 2, 260, device=DEV), torch.zeros(3, 260, 3, 3, device=DEV), form="narrow")
    y = torch.zeros(1, 4, 4, 3, device=DEV)
    with pytest.raises(ValueError, match="sizes"):
        K.conv3x3_narrow_fwd(x, torch.zeros(3, 8, 3, 3, device=DEV), 1, 4, 5, 8, 3, y)
    with pytest.raises(ValueError, match="partial"):
        K.conv3x3_narrow_bwd_weight(x, y, 1, 4, 4, 8, 3, torch.zeros(10, device=DEV), 2)
    # the C entry points refuse on their own
    lib = _lib.load()
    for args in ((None, x.data_ptr(), 1, 4, 4, 8, 3, y.data_ptr()), (x.data_ptr(), x.data_ptr(), 1, 4, 4, 6, 3, y.data_ptr()),
                 (x.data_ptr(), x.data_ptr(), 1, 4, 4, 8, 5, y.data_ptr()), (x.data_ptr(), x.data_ptr(), 1 << 9, 1 << 9, 1 << 9, 8, 3, y.data_ptr())):
        assert lib.tpgsr_conv3x3_narrow_fwd(*args, None) == -1
        assert lib.tpgsr_conv3x3_narrow_bwd_data(*args, None) == -1
    assert y.abs().sum().item() == 0
