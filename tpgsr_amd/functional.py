"""Operator-level API: every building block of the reference's networks as a differentiable function on the HIP kernels.

The fused engines (engine.py / engine_crnn.py) run whole networks as recorded plans.  This module is the same kernel
library exposed one operator at a time -- a `torch.autograd.Function` per op whose forward AND backward are C-ABI launches --
so that (i) the reference's block classes work standalone (`STNHead(x) -> (feat, ctrl)`, `TPSSpatialTransformer`,
`GruBlock`, `RecurrentResidualBlock(TL)`, `InfoGen`, `UpsampleBLock`, `mish`: SURVEY.md section 8b), and (ii) the other
`--arch` / `--tpg` choices of the reference (the _TL baseline backbones, the OPT text-prior generator) are written the way
the reference writes them, layer by layer, without a single ATen compute kernel.

Conventions: activations are fp32 CUDA tensors in NHWC order (N, H, W, C), contiguous; `to_nhwc` / `to_nchw` convert at the
module boundary.  Parameters keep the PyTorch layouts (state_dict interchange); weights are packed per call (these paths are
not the tuned hot path).  Nothing here falls back to a stock PyTorch kernel: non-CUDA inputs raise."""
from __future__ import annotations

from contextlib import contextmanager, nullcontext
from typing import Optional, Sequence, Tuple

import torch

from . import kernels as K
from .kernels import ConvGeom

F32 = torch.float32


def _chk(*ts):
    for t in ts:
        if t is None:
            continue
        if not (t.is_cuda or K.DRYRUN):
            raise RuntimeError("tpgsr_amd.functional runs on the GPU only (no CPU / stock-PyTorch fallback)")
        if t.dtype != F32:
            raise TypeError(f"tpgsr_amd.functional expects fp32 tensors, got {t.dtype}")


def _new(like, *shape):
    return torch.empty(*shape, dtype=F32, device=like.device)


# Parameter-gradient sinks (engine_functional.py, recorded mode): data_ptr of a parameter -> the fp32 buffer its gradient is ACCUMULATED
# into by the operator's own backward kernels (the slab reduce / the BatchNorm-backward finalize with accumulate = 1).  The backward then
# hands autograd `None` for that parameter: no AccumulateGrad node runs, i.e. no ATen `add_` that a recorded plan could not replay.
# Installed by grad_sinks(), read by _grad_dst() alone.
GRAD_SINK: dict = {}


@contextmanager
def grad_sinks(mapping: dict):
    """`mapping` is the sink table inside the block; the previous table comes back after it"""
    global GRAD_SINK
    prev, GRAD_SINK = GRAD_SINK, mapping
    try:
        yield mapping
    finally:
        GRAD_SINK = prev


def _grad_dst(*ps):
    """Where the gradients of a parameter and of those reduced by the same launch (its bias / beta; None entries stay None) go
    -> (destinations, accumulate, what the backward hands autograd): the sinks, accumulated into, and None for autograd where the first
    parameter has a sink; fresh tensors, overwritten and returned, otherwise.  Every operator with a parameter asks here."""
    sinks = [None if p is None else GRAD_SINK.get(p.data_ptr()) for p in ps]
    if sinks[0] is None:
        fresh = tuple(None if p is None else torch.empty_like(p, memory_format=torch.contiguous_format) for p in ps)
        return fresh, False, fresh
    if any(s is None for s, p in zip(sinks, ps) if p is not None):
        raise RuntimeError("a sunk weight gradient needs its bias gradient sunk too")
    return tuple(sinks), True, (None,) * len(ps)


def _conv_wgrad(g, x, dy, w, b=None, *, in_ld=None, in_coff=0, dy_ld=None, dy_coff=0, dy_ps=False, layout=0, gscale=1.0, geom_splits=True,
                staged=None):
    """Weight (and bias) gradient of convolution `g` over input x and output gradient dy -> (dw, db) for autograd (None where sunk).
    Slabs and reduce are a leaf of the graph: on the weight-gradient stream when a recorded plan overlaps them (K.side() is a no-op
    eagerly).  in_* / dy_*: the windows of x / dy the convolution ran on.  geom_splits=False: the legacy split count (the BiGRU's 1x1
    products).  staged = (buffer, finish): the slabs are reduced into `buffer` at once, not in the plan's batched reduce, and
    finish(destination, accumulate) reads it next on the same stream (the sub-pixel transposed convolution's fold)."""
    Z = K.wgrad_splits(g.M, g.K, g.Cout, geom=g if geom_splits else None)
    part = _new(x, Z, g.K, g.Cout)
    dbp = _new(x, Z, g.Cout) if b is not None else None
    dst, acc, ret = _grad_dst(w, b)
    with K.side():
        K.conv_wgrad(K.make_wgrad_args(K.make_conv_args(g, x, in_ld=in_ld, in_coff=in_coff), dy, part, dbp, dy_ld=dy_ld, dy_coff=dy_coff,
                                       dy_ps=dy_ps, zsplits=Z if geom_splits else 0))
        if staged is None:
            K.wgrad_reduce(part, dbp, Z, g, *dst, layout=layout, accumulate=acc, gscale=gscale)
        else:
            K.wgrad_reduce(part, None, Z, g, staged[0], None, layout=layout, accumulate=False, gscale=gscale, defer=False)
            staged[1](dst[0], acc)
    return ret


def _partials_grad(p, part, rows, n, launch=None):
    """partial sums part [rows][n] -> the gradient of parameter p for autograd (None where sunk).  launch: the kernel that fills `part`; it
    and the reduce are a side-stream section like _conv_wgrad's.  None: they are there already and the reduce stays on the caller's
    stream (PReLU: its backward kernel writes them next to dx)."""
    (dst,), acc, (ret,) = _grad_dst(p)
    with (K.side() if launch is not None else nullcontext()):
        if launch is not None:
            launch()
        K.reduce_partials(part, rows, n, dst, accumulate=acc)
    return ret


def _row_partials_grad(ps, part, rows, n, launch):
    """_partials_grad for ONE kernel that leaves the partial sums of several parameters in one row -- part [rows][n] holds the gradients
    of `ps` one behind another (a weight, then its bias; trailing columns of an absent parameter are dropped) -> a tuple for autograd
    (None where sunk).  The parameters' destinations are separate tensors and tpgsr_reduce_partials writes a row to one place (its row
    length is its row stride), so the row is reduced into a buffer of its own and one launch per parameter carries its slice on: a
    tpgsr_add into a sink, a tpgsr_copy into a fresh tensor.  One pass over the pixels for all of them is what the shared row buys."""
    dst, acc, ret = _grad_dst(*ps)
    row = _new(part, n)
    offs = [sum(q.numel() for q in ps[:i]) for i in range(len(ps))]
    with K.side():
        launch()
        K.reduce_partials(part, rows, n, row, accumulate=False)
        for q, o, d in zip(ps, offs, dst):
            if acc:
                K.add(d, row[o:o + q.numel()], q.numel(), d)
            else:
                K.copy(row[o:o + q.numel()], d, q.numel())
    return ret


def _choose_form(op, form, forms, default, unfit, hint=" or None"):
    """the `form=` argument of a wrapper with several routes -> the form to run.  An unknown name raises; None is `default`; `unfit` maps
    the forms these arguments have no route in to the reason, which raises when one of them is what would run."""
    if form is None:
        form = default
    elif form not in forms:
        raise ValueError(f"{op}: form={form!r}, expected one of {forms}{hint}")
    if form in unfit:
        raise ValueError(f"{op}: {unfit[form]}")
    return form


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


# ---- layout ---------------------------------------------------------------------------------------------------------
class _ToNHWC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _chk(x)
        N, C, H, W = x.shape
        out = _new(x, N, H, W, C)
        K.nchw_to_nhwc(_c(x), N, C, H, W, out)
        return out

    @staticmethod
    def backward(ctx, g):
        N, H, W, C = g.shape
        out = _new(g, N, C, H, W)
        K.nhwc_to_nchw(_c(g), N, C, H, W, out)
        return out


class _ToNCHW(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _chk(x)
        N, H, W, C = x.shape
        out = _new(x, N, C, H, W)
        K.nhwc_to_nchw(_c(x), N, C, H, W, out)
        return out

    @staticmethod
    def backward(ctx, g):
        N, C, H, W = g.shape
        out = _new(g, N, H, W, C)
        K.nchw_to_nhwc(_c(g), N, C, H, W, out)
        return out


def to_nhwc(x):
    return _ToNHWC.apply(x)


def to_nchw(x):
    return _ToNCHW.apply(x)


# ---- convolution / linear ------------------------------------------------------------------------------------------
def _pack(w, transposed, wscale):
    """PyTorch conv weight -> (wt_f [K][Cout_p], wt_d [KH*KW*Cout][Cin_p]); channel counts that are not multiples of 4 are
    zero-padded in the operand's row length so the 16-byte weight loads apply"""
    if transposed:
        Cin, Cout, KH, KW = w.shape
    else:
        Cout, Cin, KH, KW = w.shape
    wt_f = torch.empty(KH * KW * Cin, Cout, dtype=F32, device=w.device)
    wt_d = torch.empty(KH * KW * Cout, Cin, dtype=F32, device=w.device)
    K.pack_conv_weight(_c(w), Cout, Cin, KH, KW, wt_f, wt_d, transposed=transposed, wscale=wscale)
    if K.CONV_TERMS:
        K.make_bf_twin(wt_f, Cin)
        K.make_bf_twin(wt_d, Cout)
    return wt_f, wt_d, Cout, Cin, KH, KW


class _Conv2d(torch.autograd.Function):
    """stride-1 conv (nn.Conv2d / nn.Linear as 1x1); `transposed`: the weight is a ConvTranspose2d weight [Cin][Cout][KH][KW]
    and the op is its equivalent stride-1 conv (flipped taps) over an already zero-dilated input."""

    @staticmethod
    def forward(ctx, x, w, b, pad_h, pad_w, out_ps, transposed, wscale):
        _chk(x, w, b)
        x = _c(x)
        N, H, W, Cx = x.shape
        wt_f, wt_d, Cout, Cin, KH, KW = _pack(w, transposed, wscale)
        if Cx != Cin:
            raise ValueError(f"conv2d: input has {Cx} channels, weight expects {Cin}")
        g = ConvGeom(N, H, W, Cin, Cout, KH, KW, pad_h, pad_w)
        if g.OH <= 0 or g.OW <= 0:
            raise ValueError("conv2d: empty output")
        out = _new(x, N, 2 * g.OH, 2 * g.OW, Cout // 4) if out_ps else _new(x, N, g.OH, g.OW, Cout)
        K.conv_fwd(K.make_conv_args(g, x, wt_f, out, bias=b, out_ps=out_ps))
        ctx.save_for_backward(x, w, wt_d, b)
        ctx.cfg = (g, out_ps, transposed, wscale)
        return out

    @staticmethod
    def backward(ctx, dy):
        x, w, wt_d, b = ctx.saved_tensors
        g, out_ps, transposed, wscale = ctx.cfg
        dy = _c(dy)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = _new(x, g.N, g.H, g.W, g.Cin)
            K.conv_fwd(K.make_conv_args(g.dgrad(), dy, wt_d, dx, in_ps=out_ps))
        if ctx.needs_input_grad[1] or (b is not None and ctx.needs_input_grad[2]):
            dw, db = _conv_wgrad(g, x, dy, w, b, dy_ps=out_ps, layout=1 if transposed else 0, gscale=wscale)
        return dx, dw, db, None, None, None, None, None


def conv2d(x, w, b=None, padding=0, out_ps=False, wscale=1.0):
    ph, pw = (padding, padding) if isinstance(padding, int) else padding
    return _Conv2d.apply(x, w, b, ph, pw, bool(out_ps), False, float(wscale))


def linear(x, w, b=None, wscale=1.0):
    """x (..., Cin) -> (..., Cout) with an nn.Linear weight [Cout][Cin]"""
    lead = x.shape[:-1]
    y = conv2d(x.reshape(1, 1, -1, x.shape[-1]), w.reshape(w.shape[0], w.shape[1], 1, 1), b, 0, wscale=wscale)
    return y.reshape(*lead, w.shape[0])


class _Dilate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, sh, sw):
        _chk(x)
        x = _c(x)
        N, H, W, C = x.shape
        out = _new(x, N, (H - 1) * sh + 1, (W - 1) * sw + 1, C)
        K.dilate2d(x, N, H, W, C, sh, sw, out)
        ctx.cfg = (sh, sw)
        return out

    @staticmethod
    def backward(ctx, g):
        sh, sw = ctx.cfg
        g = _c(g)
        N, H, W, C = g.shape
        out = _new(g, N, (H + sh - 1) // sh, (W + sw - 1) // sw, C)
        K.subsample2d(g, N, H, W, C, sh, sw, out)
        return out, None, None


class _Subsample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, sh, sw):
        _chk(x)
        x = _c(x)
        N, H, W, C = x.shape
        out = _new(x, N, (H + sh - 1) // sh, (W + sw - 1) // sw, C)
        K.subsample2d(x, N, H, W, C, sh, sw, out)
        ctx.cfg = (sh, sw, H, W)
        return out

    @staticmethod
    def backward(ctx, g):
        sh, sw, H, W = ctx.cfg
        g = _c(g)
        N, OH, OW, C = g.shape
        d = _new(g, N, (OH - 1) * sh + 1, (OW - 1) * sw + 1, C)
        K.dilate2d(g, N, OH, OW, C, sh, sw, d)
        if d.shape[1] == H and d.shape[2] == W:
            return d, None, None
        full = torch.zeros(N, H, W, C, dtype=F32, device=g.device)      # rows / columns past the last sample get no gradient
        _rows_copy(d, full)
        return full, None, None


def _rows_copy(d, full):
    N, dH, dW, C = d.shape
    _, H, W, _ = full.shape
    for n in range(N):
        K.copy_strided(d[n], dW * C, 0, full[n], W * C, 0, dH, dW * C)


def subsample(x, sh, sw):
    return x if (sh == 1 and sw == 1) else _Subsample.apply(x, sh, sw)


def conv_transpose2d(x, w, stride=1, padding=0):
    """nn.ConvTranspose2d(bias=False, output_padding=0): zero-dilate the input, then the equivalent stride-1 conv"""
    sh, sw = (stride, stride) if isinstance(stride, int) else stride
    ph, pw = (padding, padding) if isinstance(padding, int) else padding
    KH, KW = w.shape[2], w.shape[3]
    xd = x if (sh == 1 and sw == 1) else _Dilate.apply(x, sh, sw)
    return _Conv2d.apply(xd, w, None, KH - 1 - ph, KW - 1 - pw, False, True, 1.0)


class _TConvK4S2SubPixel(torch.autograd.Function):
    """ConvTranspose2d(Cin, Cout, 4, 2, 1, bias=False) as the 3x3 pad-1 convolution to 4 Cout channels with the pixel-shuffle store
    (csrc/tconv4s2.hip): 36 multiply-adds per input pixel and channel pair where the zero-dilated form spends 64, and no dilated tensor.
    The weight is expanded per call (tpgsr_tconv4s2_expand); the convolution's weight gradient is reduced HERE (not in the plan's batched
    reduce: the fold reads it next on the same stream) and folded back into the [Cin][Cout][4][4] gradient (tpgsr_tconv4s2_fold_grad)."""

    @staticmethod
    def forward(ctx, x, w):
        _chk(x, w)
        x = _c(x)
        N, H, W, Cx = x.shape
        Cin, Cout = w.shape[0], w.shape[1]
        w3 = _new(x, 4 * Cout, Cin, 3, 3)
        K.tconv4s2_expand(_c(w), Cin, Cout, w3)
        wt_f, wt_d, *_ = _pack(w3, False, 1.0)
        g = ConvGeom(N, H, W, Cin, 4 * Cout, 3, 3, 1, 1)
        out = _new(x, N, 2 * H, 2 * W, Cout)
        K.conv_fwd(K.make_conv_args(g, x, wt_f, out, out_ps=True))
        ctx.save_for_backward(x, w, wt_d)
        ctx.g = g
        return out

    @staticmethod
    def backward(ctx, dy):
        x, w, wt_d = ctx.saved_tensors
        g = ctx.g
        Cin, Cout = w.shape[0], w.shape[1]
        dy = _c(dy)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = _new(x, g.N, g.H, g.W, g.Cin)
            K.conv_fwd(K.make_conv_args(g.dgrad(), dy, wt_d, dx, in_ps=True))
        if ctx.needs_input_grad[1]:
            dw3 = _new(x, 4 * Cout, Cin, 3, 3)
            dw, _ = _conv_wgrad(g, x, dy, w, dy_ps=True,
                                staged=(dw3, lambda dst, acc: K.tconv4s2_fold_grad(dw3, Cin, Cout, dst, accumulate=acc)))
        return dx, dw


class _TConvK4S2Small(torch.autograd.Function):
    """the same layer for 1 <= Cin, Cout <= 4 (LapSRN's image branch): three direct kernels, no matrix cores (csrc/tconv4s2.hip)"""
    NBLK = 512      # rows of the weight gradient's partial sums (at most one per 64 input positions)

    @staticmethod
    def forward(ctx, x, w):
        _chk(x, w)
        x, w = _c(x), _c(w)
        N, H, W, Cx = x.shape
        Cin, Cout = w.shape[0], w.shape[1]
        out = _new(x, N, 2 * H, 2 * W, Cout)
        K.tconv4s2_small_fwd(x, w, N, H, W, Cin, Cout, out)
        ctx.save_for_backward(x, w)
        return out

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        N, H, W, Cin = x.shape
        Cout = w.shape[1]
        dy = _c(dy)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            K.tconv4s2_small_bwd_data(dy, w, N, H, W, Cin, Cout, dx)
        if ctx.needs_input_grad[1]:
            nblk = max(1, min(_TConvK4S2Small.NBLK, (N * H * W + 63) // 64))
            E = Cin * Cout * 16
            part = _new(x, nblk, E)
            dw = _partials_grad(w, part, nblk, E, lambda: K.tconv4s2_small_bwd_weight(x, dy, N, H, W, Cin, Cout, part, nblk))
        return dx, dw


# (Cin, Cout) whose 3x3 Cin -> 4 Cout pixel-shuffle-store convolution -- forward, in_ps data gradient, dy_ps weight gradient -- is in the
# instantiated and tested set of the convolution kernels (the 64 -> 256 convolution of the up-sampling blocks)
TCONV_SUBPIXEL_PAIRS = frozenset({(64, 64)})
TCONV_FORMS = ("direct", "subpixel", "dilated")


def tconv_k4s2_form(Cin: int, Cout: int) -> str:
    """the form conv_transpose2d_k4s2 runs a channel pair in"""
    if Cin <= K.TCONV_SMALL_MAX_C and Cout <= K.TCONV_SMALL_MAX_C:
        return "direct"
    return "subpixel" if (Cin, Cout) in TCONV_SUBPIXEL_PAIRS else "dilated"


def conv_transpose2d_k4s2(x, w, form: Optional[str] = None):
    """nn.ConvTranspose2d(Cin, Cout, 4, stride=2, padding=1, bias=False) on an NHWC map, w [Cin][Cout][4][4] -> (N, 2H, 2W, Cout).
    Up to four channels on both sides: the direct kernels.  64 -> 64: the sub-pixel form (3x3 pixel-shuffle-store convolution on the
    matrix cores).  Any other pair: the zero-dilated form of conv_transpose2d.  form: a measurement names the form itself
    (tools/lab/lapsrn_step_time.py); a form the channel pair has no route for raises."""
    if w.dim() != 4 or tuple(w.shape[2:]) != (4, 4):
        raise ValueError(f"conv_transpose2d_k4s2: a [Cin][Cout][4][4] weight, got {tuple(w.shape)}")
    Cin, Cout = w.shape[0], w.shape[1]
    if x.dim() != 4 or x.shape[-1] != Cin:
        raise ValueError(f"conv_transpose2d_k4s2: input {tuple(x.shape)} is not (N, H, W, {Cin})")
    auto = tconv_k4s2_form(Cin, Cout)
    unfit = {f: f"no {f} route for {Cin} -> {Cout} channels" for f in ("direct", "subpixel") if f != auto}
    form = _choose_form("conv_transpose2d_k4s2", form, TCONV_FORMS, auto, unfit, hint="")
    if form == "direct":
        return _TConvK4S2Small.apply(x, w)
    if form == "subpixel":
        return _TConvK4S2SubPixel.apply(x, w)
    return conv_transpose2d(x, w, 2, 1)


def conv2d_strided(x, w, b=None, stride=(1, 1), padding=0):
    """strided conv = stride-1 conv + sub-sampling (only the small conv4_1 of the OPT feature extractor uses it)"""
    return subsample(conv2d(x, w, b, padding), stride[0], stride[1])


# ---- BatchNorm (+ fused activation) ----------------------------------------------------------------------------------
class _BatchNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, rm, rv, training, momentum, eps, act):
        _chk(x, gamma, beta)
        x = _c(x)
        C = x.shape[-1]
        M = x.numel() // C
        if training and any(ctx.needs_input_grad[:3]) and not (C % 4 == 0 and C <= 1024 and 256 % (C // 4) == 0):
            raise ValueError(f"batch_norm: the backward kernels take a channel count that is a multiple of 4 with C / 4 dividing 256, got {C}")
        dev = x.device
        scale, shift = torch.empty(C, device=dev), torch.empty(C, device=dev)
        mean, rstd = torch.empty(C, device=dev), torch.empty(C, device=dev)
        if training:
            nblk = max(1, min(1024, M // 64))
            part = torch.empty(nblk, 2, C, device=dev)
            K.bn_stats(x, M, C, part, nblk)
            K.bn_finalize(part, nblk, C, M, None, gamma, beta, rm, rv, scale, shift, mean, rstd, momentum=momentum, eps=eps)
        else:
            K.bn_finalize(None, 0, C, 0, None, gamma, beta, rm, rv, scale, shift, momentum=momentum, eps=eps, eval_mode=True)
        out = torch.empty_like(x)
        K.affine_act(x, M, C, scale, shift, act, out)
        ctx.save_for_backward(x, gamma, beta, scale, shift, mean, rstd)
        ctx.cfg = (training, act, M, C)
        return out

    @staticmethod
    def backward(ctx, dy):
        x, gamma, beta, scale, shift, mean, rstd = ctx.saved_tensors
        training, act, M, C = ctx.cfg
        if not training:
            raise RuntimeError("backward through an eval-mode BatchNorm is not supported (the reference only trains in train mode)")
        dy = _c(dy)
        dev = x.device
        nblk = max(1, min(1024, M // 64))
        part = torch.empty(nblk, 2, C, device=dev)
        coef = torch.empty(3, C, device=dev)
        dst, acc, (dgamma, dbeta) = _grad_dst(gamma, beta)
        K.bn_bwd_reduce(dy, None, x, M, C, scale, shift, mean, rstd, act, part, nblk)
        K.bn_bwd_finalize(part, nblk, C, M, gamma, mean, rstd, *dst, coef, accumulate=acc)
        dx = torch.empty_like(x)
        K.bn_bwd_apply(dy, None, x, M, C, scale, shift, act, coef, dx)
        return dx, dgamma, dbeta, None, None, None, None, None, None


def batch_norm(x, bn, training: bool, act: Optional[str] = None):
    """bn: a BatchNormParams holder (weight, bias, running_mean, running_var, momentum, eps); act fused: 'relu' | 'mish' | None.
    A training-mode call that needs a gradient takes C = 4, 8, 16, ... (a multiple of 4 with C / 4 dividing 256: the vector backward
    kernels) and raises ValueError otherwise; the backward of an eval-mode call raises RuntimeError."""
    if training and K._REC is None:      # (a recorded plan's engine counts its replays: engine_functional.py flush_counters)
        bn.num_batches_tracked += 1
    return _BatchNorm.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bool(training), bn.momentum, bn.eps, act)


# ---- elementwise -----------------------------------------------------------------------------------------------------
class _Act(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, act):
        _chk(x)
        x = _c(x)
        if x.numel() % 4:
            raise ValueError("activation: element count must be a multiple of 4")
        out = torch.empty_like(x)
        K.affine_act(x, x.numel() // 4, 4, None, None, act, out)
        ctx.save_for_backward(x)
        ctx.act = act
        return out

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dx = torch.empty_like(x)
        K.act_bwd(x, _c(dy), x.numel(), ctx.act, dx)
        return dx, None


def relu(x):
    return _Act.apply(x, "relu")


def mish(x):
    return _Act.apply(x, "mish")


def tanh(x):
    return _Act.apply(x, "tanh")


class _LeakyReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, slope):
        _chk(x)
        x = _c(x)
        out = torch.empty_like(x)
        K.leaky_relu_fwd(x, x.numel(), slope, out)
        ctx.save_for_backward(x)
        ctx.slope = slope
        return out

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dx = torch.empty_like(x)
        K.leaky_relu_bwd(x, _c(dy), x.numel(), ctx.slope, dx)
        return dx, None


def leaky_relu(x, slope: float = 0.01):
    """nn.LeakyReLU(slope): any element count; the derivative at x <= 0 is `slope` (ATen's)"""
    return _LeakyReLU.apply(x, float(slope))


class _PReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, alpha):
        _chk(x, alpha)
        x = _c(x)
        out = torch.empty_like(x)
        K.prelu_fwd(x, alpha, x.numel(), out)
        ctx.save_for_backward(x, alpha)
        return out

    @staticmethod
    def backward(ctx, dy):
        x, alpha = ctx.saved_tensors
        nb = 256
        dx = torch.empty_like(x)
        dap = torch.empty(nb, device=x.device)
        K.prelu_bwd(x, alpha, _c(dy), None, x.numel(), dx, dap, nb)
        return dx, _partials_grad(alpha, dap, nb, 1)


def prelu(x, alpha):
    return _PReLU.apply(x, alpha)


class _Add(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        _chk(a, b)
        if a.shape != b.shape:
            raise ValueError(f"add: {tuple(a.shape)} vs {tuple(b.shape)}")
        out = torch.empty_like(a, memory_format=torch.contiguous_format)
        K.add(_c(a), _c(b), a.numel(), out)
        return out

    @staticmethod
    def backward(ctx, g):
        return g, g


def add(a, b):
    return _Add.apply(a, b)


class _ScaledAdd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, alpha):
        _chk(a, b)
        if a.shape != b.shape:
            raise ValueError(f"scaled_add: {tuple(a.shape)} vs {tuple(b.shape)}")
        a, b = _c(a), _c(b)
        C = a.shape[-1]
        out = torch.empty_like(a)
        K.scaled_add(a, C, 0, b, C, 0, alpha, out, C, 0, a.numel() // C, C)
        ctx.alpha = alpha
        return out

    @staticmethod
    def backward(ctx, g):
        da = None
        if ctx.needs_input_grad[0]:
            g = _c(g)
            C = g.shape[-1]
            da = torch.empty_like(g)
            K.scaled_add(g, C, 0, None, 0, 0, ctx.alpha, da, C, 0, g.numel() // C, C)
        return da, (g if ctx.needs_input_grad[1] else None), None      # (the second term is passed through: no launch)


def scaled_add(a, b, alpha: float):
    """alpha * a + b (the 0.2-scaled residuals of ESRGAN's blocks, model/esrgan.py:36, :52): one launch forward, one (alpha * g) backward"""
    return _ScaledAdd.apply(a, b, float(alpha))


class _Fork(torch.autograd.Function):
    """x -> n views of x for a tensor with n consumers (the identity branch of a residual block, a text-prior map fed to every block):
    the incoming gradients are summed here by ONE launch (tpgsr_add for two, tpgsr_add_n for up to eight, left to right in consumer
    order), not by autograd's own accumulation (ATen kernels -- and invisible to a recorded plan)"""

    @staticmethod
    def forward(ctx, x, n):
        _chk(x)
        ctx.set_materialize_grads(False)      # an unused consumer hands `None` to backward, not a zero tensor filled by an ATen kernel
        return tuple(x.view_as(x) for _ in range(n))

    @staticmethod
    def backward(ctx, *gs):
        live = [_c(g) for g in gs if g is not None]
        if len(live) <= 1:
            return (live[0] if live else None), None      # a single survivor is passed through: no launch
        out = torch.empty_like(live[0], memory_format=torch.contiguous_format)
        if len(live) == 2:
            K.add(live[0], live[1], out.numel(), out)
        else:
            K.add_n(live, out.numel(), out)
        return out, None


def fork(x, n: int = 2):
    """n views of x, one per consumer (2 <= n <= 8); their gradients are summed by one HIP launch in the backward pass"""
    if not 2 <= n <= 8:
        raise ValueError(f"fork: 2 to 8 consumers, got {n}")
    return _Fork.apply(x, int(n))


class _Cat(torch.autograd.Function):
    """torch.cat(xs, channel axis) in NHWC = interleaving channel slices"""

    @staticmethod
    def forward(ctx, *xs):
        _chk(*xs)
        lead = xs[0].shape[:-1]
        cs = [x.shape[-1] for x in xs]
        if any(x.shape[:-1] != lead for x in xs):
            raise ValueError("cat: leading dimensions differ")
        Ct = sum(cs)
        out = _new(xs[0], *lead, Ct)
        M = out.numel() // Ct
        off = 0
        for x, c in zip(xs, cs):
            K.copy_strided(_c(x), c, 0, out, Ct, off, M, c)
            off += c
        ctx.cs = cs
        return out

    @staticmethod
    def backward(ctx, g):
        g = _c(g)
        Ct = g.shape[-1]
        M = g.numel() // Ct
        outs, off = [], 0
        for c in ctx.cs:
            d = _new(g, *g.shape[:-1], c)
            K.copy_strided(g, Ct, off, d, c, 0, M, c)
            outs.append(d)
            off += c
        return tuple(outs)


def cat(xs: Sequence[torch.Tensor]):
    return _Cat.apply(*xs)


# ---- residual dense block (ESRGAN's ResidualDenseBlock_5C, model/esrgan.py:16-36) -------------------------------------------------
class _DenseBlock(torch.autograd.Function):
    """y = res_scale * conv5([x, x1, x2, x3, x4]) + x with x_k = LeakyReLU(conv_k([x, x1 .. x_{k-1}])), on ONE concatenation buffer
    D [M][nf + 4 gc]: convolution k reads the channel prefix [0, Cin_k) of D and writes the window behind it (input and output share the
    buffer, the windows are disjoint), tpgsr_leaky_relu_window activates the window in place.  No concatenation is ever copied: one
    tpgsr_copy_strided puts x into the buffer.

    The backward pass works in place the same way on a gradient buffer G [M][nf + 4 gc]: conv5's data gradient fills it, then for k = 4 .. 1
    tpgsr_dense_bwd_step masks window k by the activation's derivative (read from D's POST-activation values: same sign for slope > 0; the
    first call is mask-only, T = NULL), conv k's data gradient goes into a dense T_k [M][Cin_k], and the next step adds T_k to G's prefix
    while it masks window k - 1.  The last step writes dx = (G[:, :nf] + T_1) + dy.  res_scale is applied to dy by one tpgsr_scaled_add
    launch (it is NOT folded into conv5's packed weight).  Window k of G is final once masked -- later steps only touch the columns in
    front of it -- so the weight-gradient launches on the side stream read it unordered with the caller's stream moving on; G and every T
    are the operator's own allocations (a recorded plan keeps them alive)."""

    @staticmethod
    def forward(ctx, x, slope, res_scale, *wb):
        ws, bs = wb[:5], wb[5:]
        _chk(x, *ws, *bs)
        x = _c(x)
        N, H, W, nf = x.shape
        gc = ws[0].shape[0]
        Ct = nf + 4 * gc
        M = N * H * W
        D = _new(x, N, H, W, Ct)
        K.copy_strided(x, nf, 0, D, Ct, 0, M, nf)
        geoms, wds = [], []
        for k in range(4):
            Cin = nf + k * gc
            wt_f, wt_d, *_ = _pack(ws[k], False, 1.0)
            g = ConvGeom(N, H, W, Cin, gc, 3, 3, 1, 1)
            K.conv_fwd(K.make_conv_args(g, D, wt_f, D, bias=bs[k], in_ld=Ct, out_ld=Ct, out_coff=Cin))
            K.leaky_relu_window(D, Ct, Cin, gc, M, slope)
            geoms.append(g)
            wds.append(wt_d)
        wt_f, wt_d, *_ = _pack(ws[4], False, 1.0)
        g = ConvGeom(N, H, W, Ct, nf, 3, 3, 1, 1)
        y = _new(x, N, H, W, nf)
        K.conv_fwd(K.make_conv_args(g, D, wt_f, y, bias=bs[4]))
        K.scaled_add(y, nf, 0, D, Ct, 0, res_scale, y, nf, 0, M, nf)      # in place on x5: the backward needs D only
        geoms.append(g)
        wds.append(wt_d)
        ctx.save_for_backward(D, *ws, *wds, *bs)
        ctx.cfg = (geoms, slope, res_scale, nf, gc)
        return y

    @staticmethod
    def backward(ctx, dy):
        D, *rest = ctx.saved_tensors
        ws, wds, bs = rest[:5], rest[5:10], rest[10:]
        geoms, slope, res_scale, nf, gc = ctx.cfg
        dy = _c(dy)
        N, H, W, Ct = D.shape
        M = N * H * W
        dws, dbs = [None] * 5, [None] * 5

        def wgrad(k, dy, dy_ld=None, dy_coff=0):
            if ctx.needs_input_grad[3 + k] or (bs[k] is not None and ctx.needs_input_grad[8 + k]):
                dws[k], dbs[k] = _conv_wgrad(geoms[k], D, dy, ws[k], bs[k], in_ld=Ct, dy_ld=dy_ld, dy_coff=dy_coff)
        dx5 = torch.empty_like(dy)
        K.scaled_add(dy, nf, 0, None, 0, 0, res_scale, dx5, nf, 0, M, nf)
        G = _new(D, N, H, W, Ct)
        K.conv_fwd(K.make_conv_args(geoms[4].dgrad(), dx5, wds[4], G))
        wgrad(4, dx5)
        T = None
        for k in (3, 2, 1, 0):
            g = geoms[k]
            Cin = g.Cin
            K.dense_bwd_step(G, Ct, T, Cin + gc, D, Cin, gc, slope, M)      # (k = 3: mask only, every column of G is conv5's alone so far)
            wgrad(k, G, Ct, Cin)
            T = _new(D, N, H, W, Cin)
            K.conv_fwd(K.make_conv_args(g.dgrad(), G, wds[k], T, in_ld=Ct, in_coff=Cin))
        dx = torch.empty_like(dy)
        K.dense_bwd_step(G, Ct, T, nf, None, 0, 0, slope, M, skip=dy, dx=dx)
        return (dx, None, None, *dws, *dbs)


DENSE_FORMS = ("inplace", "composed")


def _dense_block_composed(x, ws, bs, slope, res_scale):
    """the block as model/rdn.py composes its dense layers: fork / cat / conv2d / leaky_relu, the scaled residual by scaled_add"""
    cur, skip = fork(x)
    for k in range(4):
        cur, keep = fork(cur)
        cur = cat([keep, leaky_relu(conv2d(cur, ws[k], bs[k], 1), slope)])
    return scaled_add(conv2d(cur, ws[4], bs[4], 1), skip, res_scale)


def dense_block(x, weights, biases=None, slope: float = 0.2, res_scale: float = 0.2, form: Optional[str] = None):
    """ResidualDenseBlock_5C (reference model/esrgan.py:16-36) on an NHWC map x (N, H, W, nf): weights = five 3x3 convolution weights
    [gc | nf][nf + k gc][3][3], biases = five vectors, or None entries / None.  form "inplace": the block on one concatenation buffer
    (_DenseBlock; channel counts that are multiples of 4); "composed": the same mathematics over fork / cat / conv2d / leaky_relu;
    None: in place where the channel counts allow it, composed otherwise."""
    ws = list(weights)
    bs = [None] * 5 if biases is None else list(biases)
    if len(ws) != 5 or len(bs) != 5:
        raise ValueError("dense_block: five convolution weights (and five biases or None)")
    if x.dim() != 4:
        raise ValueError(f"dense_block: input {tuple(x.shape)} is not (N, H, W, nf)")
    nf, gc = x.shape[-1], ws[0].shape[0]
    for k, w in enumerate(ws):
        want = (nf if k == 4 else gc, nf + k * gc, 3, 3)
        if tuple(w.shape) != want:
            raise ValueError(f"dense_block: weight {k + 1} is {tuple(w.shape)}, expected {want}")
    fits = nf % 4 == 0 and gc % 4 == 0
    unfit = {} if fits else {"inplace": f"the in-place form takes channel counts that are multiples of 4, got nf {nf}, gc {gc}"}
    form = _choose_form("dense_block", form, DENSE_FORMS, DENSE_DEFAULT_FORM if fits else "composed", unfit)
    if form == "composed":
        return _dense_block_composed(x, ws, bs, float(slope), float(res_scale))
    return _DenseBlock.apply(x, float(slope), float(res_scale), *ws, *bs)


# the form `form=None` runs where both fit: decided by tools/lab/rrdb_step_time.py (profiles/rrdb_step_time.md)
DENSE_DEFAULT_FORM = "inplace"


# ---- residual block (EDSR's _Residual_Block, model/edsr.py:18-32) -------------------------------------------------------------------
class _ResBlock(torch.autograd.Function):
    """y = res_scale * conv2(relu(conv1(x))) + x, two bias-free 3x3 convolutions over C channels (a multiple of 4).

    Forward: conv1 with ReLU in its epilogue (out_act) writes h, which is saved; conv2 writes r; one tpgsr_scaled_add forms
    res_scale * r + x in place on r -- a rounded product, then a rounded sum: ATen's `output *= 0.1; torch.add(output, identity)`.

    Backward: g = res_scale * dy by one tpgsr_scaled_add (b = NULL).  res_scale is NOT folded into conv2's packed weight (`wscale`): that
    would scale the forward operand too -- w2 * 0.1 rounded before the products instead of the rounded product r * 0.1 -- and the
    weight-gradient scale alone (`gscale`) would leave the data gradient unscaled.  conv2's data gradient stores dz = da * relu'(h) on its
    way out (tpgsr_conv_args.bnb_y = h, bnb_act = RELU, bnb_store_dz, no bn_partial): h is the POST-activation map, positive exactly where
    the pre-activation is, and the derivative at 0 is 0 (ATen's threshold_backward).  Where the launch has no such epilogue -- the fp32
    kernels of policy f32 -- tpgsr_act_bwd runs behind the data gradient, in place.  conv1's data gradient gives T, dx = dy + T by tpgsr_add.
    g, dz and T are the operator's own allocations, written once: the weight-gradient launches on the side stream read g / dz unordered with
    the caller's stream moving on (a recorded plan keeps them alive)."""

    @staticmethod
    def forward(ctx, x, w1, w2, res_scale):
        _chk(x, w1, w2)
        x = _c(x)
        N, H, W, C_ = x.shape
        M = N * H * W
        g = ConvGeom(N, H, W, C_, C_, 3, 3, 1, 1)
        wf1, wd1, *_ = _pack(w1, False, 1.0)
        wf2, wd2, *_ = _pack(w2, False, 1.0)
        h = torch.empty_like(x)
        K.conv_fwd(K.make_conv_args(g, x, wf1, h, out_act="relu"))
        y = torch.empty_like(x)
        K.conv_fwd(K.make_conv_args(g, h, wf2, y))
        K.scaled_add(y, C_, 0, x, C_, 0, res_scale, y, C_, 0, M, C_)
        ctx.save_for_backward(x, h, w1, w2, wd1, wd2)
        ctx.cfg = (g, res_scale)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, h, w1, w2, wd1, wd2 = ctx.saved_tensors
        g, res_scale = ctx.cfg
        dy = _c(dy)
        C_, M = g.Cin, g.M
        dw1 = dw2 = dx = None
        gr = torch.empty_like(dy)
        K.scaled_add(dy, C_, 0, None, 0, 0, res_scale, gr, C_, 0, M, C_)
        if ctx.needs_input_grad[2]:
            dw2, _ = _conv_wgrad(g, h, gr, w2)
        dz = torch.empty_like(dy)
        if K.bnb_fusable(C_) and getattr(wd2, "_tpgsr_twin", None) is not None:
            K.conv_fwd(K.make_conv_args(g.dgrad(), gr, wd2, dz, bnb=dict(y=h, act="relu", store_dz=True)))
        else:
            K.conv_fwd(K.make_conv_args(g.dgrad(), gr, wd2, dz))
            K.act_bwd(h, dz, dz.numel(), "relu", dz)
        if ctx.needs_input_grad[1]:
            dw1, _ = _conv_wgrad(g, x, dz, w1)
        if ctx.needs_input_grad[0]:
            T = torch.empty_like(dy)
            K.conv_fwd(K.make_conv_args(g.dgrad(), dz, wd1, T))
            dx = torch.empty_like(dy)
            K.add(dy, T, dx.numel(), dx)
        return dx, dw1, dw2, None


RES_FORMS = ("fused", "composed")


def _res_block_composed(x, w1, w2, res_scale):
    """the reference's mathematics over the existing operators"""
    cur, skip = fork(x)
    return scaled_add(conv2d(relu(conv2d(cur, w1, None, 1)), w2, None, 1), skip, res_scale)


def res_block(x, w1, w2, res_scale: float = 0.1, form: Optional[str] = None):
    """_Residual_Block (reference model/edsr.py:18-32) on an NHWC map x (N, H, W, C): res_scale * conv2(relu(conv1(x))) + x with two
    bias-free 3x3 convolution weights [C][C][3][3].  form "fused": one operator with a hand-written backward (_ResBlock; C a multiple
    of 4); "composed": the same mathematics over fork / conv2d / relu / scaled_add; None: RES_DEFAULT_FORM (the composed form, see there)
    where the channel count allows it, composed otherwise.  The two forms give the same bits.  Every refusal comes before a launch."""
    if x.dim() != 4:
        raise ValueError(f"res_block: input {tuple(x.shape)} is not (N, H, W, C)")
    C_ = x.shape[-1]
    for k, w in enumerate((w1, w2)):
        if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3):
            raise ValueError(f"res_block: weight {k + 1} is {tuple(w.shape)}, expected a 3x3 convolution weight [C][C][3][3]")
        if tuple(w.shape[:2]) != (C_, C_):
            raise ValueError(f"res_block: input has {C_} channels, weight {k + 1} is {tuple(w.shape)}")
    fits = C_ % 4 == 0
    unfit = {} if fits else {"fused": f"the fused form takes a channel count that is a multiple of 4, got {C_} (use form='composed')"}
    form = _choose_form("res_block", form, RES_FORMS, RES_DEFAULT_FORM if fits else "composed", unfit)
    if form == "composed":
        return _res_block_composed(x, w1, w2, float(res_scale))
    return _ResBlock.apply(x, w1, w2, float(res_scale))


# the form `form=None` runs: decided by tools/lab/edsr_step_time.py (profiles/edsr_step_time.md).  The fused form LOST that measurement --
# the activation-backward epilogue costs the data-gradient convolution more than the tpgsr_act_bwd pass it replaces, and the ReLU pass the
# forward saves is within the noise -- so it stays behind form="fused" and the default is the composed form.
RES_DEFAULT_FORM = "composed"


# ---- direct 3x3 convolution to <= 4 channels (EDSR's conv_output, model/edsr.py:57) ---------------------------------------------------
class _Conv2dNarrow(torch.autograd.Function):
    """3x3 pad-1 bias-free convolution to 1 .. 4 output channels on the direct kernels (csrc/conv_narrow.hip): the weight is read as
    PyTorch stores it (nothing is packed), plain fp32 arithmetic under every policy.  The weight gradient's partial sums are finished by
    tpgsr_reduce_partials on the side stream (into the sink in a recorded plan)."""

    @staticmethod
    def forward(ctx, x, w):
        _chk(x, w)
        x, w = _c(x), _c(w)
        N, H, W, Cin = x.shape
        Cout = w.shape[0]
        y = _new(x, N, H, W, Cout)
        K.conv3x3_narrow_fwd(x, w, N, H, W, Cin, Cout, y)
        ctx.save_for_backward(x, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        N, H, W, Cin = x.shape
        Cout = w.shape[0]
        dy = _c(dy)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            K.conv3x3_narrow_bwd_data(dy, w, N, H, W, Cin, Cout, dx)
        if ctx.needs_input_grad[1]:
            nblk = K.narrow_wgrad_blocks(N, H, W)
            E = Cout * Cin * 9
            part = _new(x, nblk, E)
            dw = _partials_grad(w, part, nblk, E, lambda: K.conv3x3_narrow_bwd_weight(x, dy, N, H, W, Cin, Cout, part, nblk))
        return dx, dw


NARROW_FORMS = ("narrow", "matrix")


def conv2d_narrow(x, w, form: Optional[str] = None):
    """nn.Conv2d(Cin, Cout <= 4, 3, padding=1, bias=False) on an NHWC map.  form "narrow": the direct kernels (Cin a multiple of 4 up to
    256); "matrix": conv2d(x, w, None, 1), the matrix-core route with Cout padded to a tile; None: NARROW_DEFAULT_FORM."""
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or not 1 <= w.shape[0] <= K.NARROW_MAX_COUT:
        raise ValueError(f"conv2d_narrow: a [Cout <= {K.NARROW_MAX_COUT}][Cin][3][3] weight, got {tuple(w.shape)}")
    Cin = w.shape[1]
    if x.dim() != 4 or x.shape[-1] != Cin:
        raise ValueError(f"conv2d_narrow: input {tuple(x.shape)} is not (N, H, W, {Cin})")
    unfit = {"narrow": f"the direct kernels take an input channel count that is a multiple of 4 up to {K.NARROW_MAX_CIN}, "
                       f"got {Cin} (use form='matrix')"} if (Cin % 4 or not 4 <= Cin <= K.NARROW_MAX_CIN) else {}
    if _choose_form("conv2d_narrow", form, NARROW_FORMS, NARROW_DEFAULT_FORM, unfit) == "matrix":
        return conv2d(x, w, None, 1)
    return _Conv2dNarrow.apply(x, w)


# the form `form=None` runs: decided by tools/lab/edsr_step_time.py (profiles/edsr_step_time.md)
NARROW_DEFAULT_FORM = "narrow"


# ---- direct 5x5 convolution to <= 4 channels, optional bias (SRCNN's conv3, model/srcnn.py) -----------------------------------------
class _Conv2dNarrow5(torch.autograd.Function):
    """5x5 pad-2 convolution to 1 .. 4 output channels on the direct kernels (csrc/conv_narrow5.hip): the weight is read as PyTorch stores
    it (nothing is packed), plain fp32 arithmetic under every policy.  One launch writes the partial sums of the weight AND the bias
    gradient; tpgsr_reduce_partials finishes them on the side stream (_row_partials_grad: into the sinks in a recorded plan)."""

    @staticmethod
    def forward(ctx, x, w, b):
        _chk(x, w, b)
        x, w = _c(x), _c(w)
        N, H, W, Cin = x.shape
        Cout = w.shape[0]
        y = _new(x, N, H, W, Cout)
        K.conv5x5_narrow_fwd(x, w, b, N, H, W, Cin, Cout, y)
        ctx.save_for_backward(x, w, b)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, b = ctx.saved_tensors
        N, H, W, Cin = x.shape
        Cout = w.shape[0]
        dy = _c(dy)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            K.conv5x5_narrow_bwd_data(dy, w, N, H, W, Cin, Cout, dx)
        if ctx.needs_input_grad[1] or (b is not None and ctx.needs_input_grad[2]):
            nblk, E = K.narrow5_wgrad_blocks(N, H, W), K.narrow5_row(Cin, Cout)
            part = _new(x, nblk, E)
            dw, *db = _row_partials_grad((w,) if b is None else (w, b), part, nblk, E,
                                         lambda: K.conv5x5_narrow_bwd_weight(x, dy, N, H, W, Cin, Cout, part, nblk))
            db = db[0] if db else None
        return dx, dw, db


def conv2d_narrow5x5(x, w, b=None, form: Optional[str] = None):
    """nn.Conv2d(Cin, Cout <= 4, 5, padding=2) on an NHWC map, b: the bias [Cout] or None.  form "narrow": the direct kernels (Cin a
    multiple of 4 up to 64); "matrix": conv2d(x, w, b, 2), the matrix-core route with Cout padded to a tile; None: NARROW5_DEFAULT_FORM.
    Every refusal comes before a launch."""
    if w.dim() != 4 or tuple(w.shape[2:]) != (5, 5) or not 1 <= w.shape[0] <= K.NARROW5_MAX_COUT:
        raise ValueError(f"conv2d_narrow5x5: a [Cout <= {K.NARROW5_MAX_COUT}][Cin][5][5] weight, got {tuple(w.shape)}")
    Cout, Cin = w.shape[:2]
    if x.dim() != 4 or x.shape[-1] != Cin:
        raise ValueError(f"conv2d_narrow5x5: input {tuple(x.shape)} is not (N, H, W, {Cin})")
    if b is not None and tuple(b.shape) != (Cout,):
        raise ValueError(f"conv2d_narrow5x5: bias {tuple(b.shape)} is not ({Cout},)")
    unfit = {"narrow": f"the direct kernels take an input channel count that is a multiple of 4 up to {K.NARROW5_MAX_CIN}, "
                       f"got {Cin} (use form='matrix')"} if (Cin % 4 or not 4 <= Cin <= K.NARROW5_MAX_CIN) else {}
    if _choose_form("conv2d_narrow5x5", form, NARROW_FORMS, NARROW5_DEFAULT_FORM, unfit) == "matrix":
        return conv2d(x, w, b, 2)
    return _Conv2dNarrow5.apply(x, w, b)


# the form `form=None` runs: decided by tools/lab/srcnn_step_time.py (profiles/srcnn_step_time.md)
NARROW5_DEFAULT_FORM = "narrow"


# ---- pooling / resampling -------------------------------------------------------------------------------------------------
class _MaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k, s, p):
        _chk(x)
        x = _c(x)
        N, H, W, C = x.shape
        OH, OW = (H + 2 * p[0] - k[0]) // s[0] + 1, (W + 2 * p[1] - k[1]) // s[1] + 1
        out = _new(x, N, OH, OW, C)
        K.pool2d_fwd(x, N, H, W, C, None, None, "none", k, s, p, out)
        ctx.save_for_backward(x)
        ctx.cfg = (k, s, p)
        return out

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        k, s, p = ctx.cfg
        N, H, W, C = x.shape
        dx = torch.empty_like(x)
        K.pool2d_bwd(x, _c(g), N, H, W, C, None, None, "none", k, s, p, dx)
        return dx, None, None, None


def max_pool2d(x, kernel, stride=None, padding=0):
    k = (kernel, kernel) if isinstance(kernel, int) else tuple(kernel)
    s = k if stride is None else ((stride, stride) if isinstance(stride, int) else tuple(stride))
    p = (padding, padding) if isinstance(padding, int) else tuple(padding)
    return _MaxPool.apply(x, k, s, p)


class _Nearest(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, s):
        _chk(x)
        x = _c(x)
        N, H, W, C = x.shape
        out = _new(x, N, H * s, W * s, C)
        K.resize_nearest_fwd(x, N, H, W, C, s, out)
        ctx.cfg = (N, H, W, C, s)
        return out

    @staticmethod
    def backward(ctx, g):
        N, H, W, C, s = ctx.cfg
        dx = _new(g, N, H, W, C)
        K.resize_nearest_bwd(_c(g), N, H, W, C, s, dx)
        return dx, None


def upsample_nearest(x, scale: int):
    """F.interpolate(x, scale_factor=scale) (mode 'nearest')"""
    return _Nearest.apply(x, int(scale))


class _Bilinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, OH, OW):
        _chk(x)
        x = _c(x)
        N, H, W, C = x.shape
        out = _new(x, N, OH, OW, C)
        K.resize_bilinear_fwd(x, N, H, W, C, OH, OW, out)
        ctx.cfg = (N, H, W, C, OH, OW)
        return out

    @staticmethod
    def backward(ctx, g):
        N, H, W, C, OH, OW = ctx.cfg
        dx = _new(g, N, H, W, C)
        K.resize_bilinear_bwd(_c(g), N, H, W, C, OH, OW, dx)
        return dx, None, None


def interpolate_bilinear(x, size: Tuple[int, int]):
    """F.interpolate(x, size, mode='bilinear', align_corners=True)"""
    return _Bilinear.apply(x, int(size[0]), int(size[1]))


class _HMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _chk(x)
        x = _c(x)
        N, H, W, C = x.shape
        out = _new(x, N, W, C)
        K.hreduce(x, N, H, W, C, 1.0 / H, out)
        ctx.cfg = (N, H, W, C)
        return out

    @staticmethod
    def backward(ctx, g):
        N, H, W, C = ctx.cfg
        dx = _new(g, N, H, W, C)
        K.hbroadcast(_c(g), N, H, W, C, 1.0 / H, dx)
        return dx


def mean_over_height(x):
    """nn.AdaptiveAvgPool2d((None, 1)) applied to the (b, w, c, h) permutation of a feature map: (N, H, W, C) -> (N, W, C)"""
    return _HMean.apply(x)


# ---- bidirectional GRU over one spatial axis (GruBlock, model/tsrn.py:491-508) --------------------------------------------
class _GruProj(torch.autograd.Function):
    """gi [N][H][W][6U] = x W_ih^T + b_ih for both directions (two MFMA 1x1 convs into the two column halves; U = hidden size)"""

    @staticmethod
    def forward(ctx, x, w0, w1, b0, b1):
        _chk(x, w0, w1, b0, b1)
        x = _c(x)
        N, H, W, Cin = x.shape
        G = w0.shape[0]
        gi = _new(x, N, H, W, 2 * G)
        packs = []
        for d, (w, b) in enumerate(((w0, b0), (w1, b1))):
            wt_f, wt_d, *_ = _pack(w.reshape(G, Cin, 1, 1), False, 1.0)
            K.conv_fwd(K.make_conv_args(ConvGeom(N, H, W, Cin, G), x, wt_f, gi, bias=b, out_ld=2 * G, out_coff=d * G))
            packs.append(wt_d)
        ctx.save_for_backward(x, *packs, w0, w1, b0, b1)
        ctx.cfg = (N, H, W, Cin, G)
        return gi

    @staticmethod
    def backward(ctx, dgi):
        x, wd0, wd1, w0, w1, b0, b1 = ctx.saved_tensors
        N, H, W, Cin, G = ctx.cfg
        dgi = _c(dgi)
        outs = []
        dx = None
        for d, (wt_d, w, b) in enumerate(((wd0, w0, b0), (wd1, w1, b1))):
            outs.append(_conv_wgrad(ConvGeom(N, H, W, Cin, G), x, dgi, w, b, dy_ld=2 * G, dy_coff=d * G, geom_splits=False))
            if ctx.needs_input_grad[0]:
                t = _new(x, N, H, W, Cin)
                K.conv_fwd(K.make_conv_args(ConvGeom(N, H, W, G, Cin), dgi, wt_d, t, in_ld=2 * G, in_coff=d * G))
                if dx is None:
                    dx = t
                else:
                    K.add(dx, t, dx.numel(), dx)
        return dx, outs[0][0], outs[1][0], outs[0][1], outs[1][1]


class _GruCore(torch.autograd.Function):
    """h [N][H][W][2U] = BiGRU scan over gi [N][H][W][6U]; U from weight_hh_l0's shape [3U][U] (32 or 64: kernels.GRU_HIDDEN)"""

    @staticmethod
    def forward(ctx, gi, whh0, whh1, bhh0, bhh1, axis):
        _chk(gi, whh0, whh1, bhh0, bhh1)
        gi = _c(gi)
        N, H, W, G2 = gi.shape
        U = whh0.shape[1]
        K.check_gru_hidden(U)          # (the refusal comes from the host, before anything is launched)
        if G2 != 6 * U or tuple(whh0.shape) != (3 * U, U) or tuple(whh1.shape) != (3 * U, U):
            raise ValueError(f"BiGRU scan: gi has {G2} columns and weight_hh is {tuple(whh0.shape)}; expected {6 * U} and ({3 * U}, {U})")
        dev = gi.device
        whh = torch.empty(2, 3 * U, U, device=dev)
        bhh = torch.empty(2, 3 * U, device=dev)
        for d, (w, b) in enumerate(((whh0, bhh0), (whh1, bhh1))):
            K.copy(_c(w), whh[d], 3 * U * U)
            K.copy(_c(b), bhh[d], 3 * U)
        h = _new(gi, N, H, W, 2 * U)
        gates = _new(gi, N, H, W, 8 * U)
        K.bigru_fwd(gi, whh, bhh, N, H, W, axis, h, gates, hidden=U)
        ctx.save_for_backward(gates, h, whh, whh0, whh1, bhh0, bhh1)
        ctx.cfg = (N, H, W, axis, U)
        return h

    @staticmethod
    def backward(ctx, dh):
        gates, h, whh, *params = ctx.saved_tensors
        N, H, W, axis, U = ctx.cfg
        dgi, dgh = _new(h, N, H, W, 6 * U), _new(h, N, H, W, 6 * U)
        K.bigru_bwd(gates, h, _c(dh), None, whh, N, H, W, axis, dgi, dgh, hidden=U)
        res = []
        for d in range(2):
            sgn = 1 if d == 0 else -1
            # dW_hh[d] = dgh[:, d]^T h_prev(d): h shifted one step against the scan direction (engine.GruLayer.bwd)
            gh = ConvGeom(N, H, W, U, 3 * U, 1, 1, sgn if axis == 1 else 0, sgn if axis == 0 else 0, H, W)
            res.append(_conv_wgrad(gh, h, dgh, params[d], params[2 + d], in_ld=2 * U, in_coff=U * d, dy_ld=6 * U, dy_coff=3 * U * d,
                                   geom_splits=False))
        return dgi, res[0][0], res[1][0], res[0][1], res[1][1], None


def bigru(x, gru, axis: int):
    """bidirectional GRU (hidden size U = 32 or 64, read from weight_hh_l0) along W (axis 0) or H (axis 1) of an NHWC map;
    gru: a GRUParams holder.  Returns [N][H][W][2U]."""
    K.check_gru_hidden(gru.weight_hh_l0.shape[1])
    gi = _GruProj.apply(x, gru.weight_ih_l0, gru.weight_ih_l0_reverse, gru.bias_ih_l0, gru.bias_ih_l0_reverse)
    return _GruCore.apply(gi, gru.weight_hh_l0, gru.weight_hh_l0_reverse, gru.bias_hh_l0, gru.bias_hh_l0_reverse, axis)


# ---- STN: TPS grid + bilinear sampler (model/tps_spatial_transformer.py:97-112) --------------------------------------------
class _TpsGrid(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ctrl, inv_kernel, coord_repr, HW):
        _chk(ctrl, inv_kernel, coord_repr)
        ctrl = _c(ctrl)
        N, NC = ctrl.shape[0], ctrl.shape[1]
        grid, src = _new(ctrl, N, HW, 2), _new(ctrl, N, HW, 2)
        K.tps_grid_fwd(ctrl, inv_kernel, coord_repr, N, HW, NC, grid, src)
        ctx.save_for_backward(src, inv_kernel, coord_repr)
        ctx.cfg = (N, HW, NC)
        ctx.mark_non_differentiable(src)
        return grid, src

    @staticmethod
    def backward(ctx, dgrid, _dsrc):
        src, inv_kernel, coord_repr = ctx.saved_tensors
        N, HW, NC = ctx.cfg
        dctrl = _new(src, N, NC, 2)
        K.tps_grid_bwd(_c(dgrid), src, inv_kernel, coord_repr, N, HW, NC, dctrl)
        return dctrl, None, None, None


class _GridSample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, grid, OH, OW, align_corners):
        _chk(x, grid)
        x, grid = _c(x), _c(grid)
        N, H, W, C = x.shape
        out = _new(x, N, OH, OW, C)
        K.grid_sample_fwd(x, grid, N, H, W, C, OH, OW, align_corners, out)
        ctx.save_for_backward(x, grid)
        ctx.cfg = (N, H, W, C, OH, OW, align_corners)
        return out

    @staticmethod
    def backward(ctx, g):
        x, grid = ctx.saved_tensors
        N, H, W, C, OH, OW, ac = ctx.cfg
        din = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dgrid = torch.empty_like(grid) if ctx.needs_input_grad[1] else None
        K.grid_sample_bwd(x, grid, _c(g), N, H, W, C, OH, OW, ac, din, dgrid)
        return din, dgrid, None, None, None


def tps_grid(ctrl, inv_kernel, coord_repr, HW):
    return _TpsGrid.apply(ctrl, inv_kernel, coord_repr, HW)


def grid_sample(x, grid, out_hw, align_corners=False):
    return _GridSample.apply(x, grid, int(out_hw[0]), int(out_hw[1]), bool(align_corners))


# ---- evaluation-only helpers of the ASTER recognizer (model/recognizer/*) -------------------------------------------------
class PackedLinear:
    """y = x W^T + b with the weight packed (and split, under the bf16 matrix-core policies) ONCE: decode loops call the same
    nn.Linear a hundred times.  No autograd (evaluation paths only)."""

    def __init__(self, w: torch.Tensor, b: Optional[torch.Tensor] = None):
        _chk(w, b)
        self.Cout, self.Cin = w.shape
        self.wt_f, _, _, _, _, _ = _pack(_c(w.detach()).reshape(self.Cout, self.Cin, 1, 1), False, 1.0)
        self.b = None if b is None else _c(b.detach())

    def __call__(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """out: optional contiguous (rows, Cout) destination (a row block of a decode loop's result)"""
        _chk(x, out)
        x = _c(x)
        rows = x.numel() // self.Cin
        if out is None:
            out = _new(x, rows, self.Cout)
        elif not out.is_contiguous() or out.numel() != rows * self.Cout:
            raise ValueError(f"PackedLinear: out must be a contiguous ({rows}, {self.Cout}) tensor")
        K.conv_fwd(K.make_conv_args(ConvGeom(1, 1, rows, self.Cin, self.Cout), x, self.wt_f, out, bias=self.b))
        return out


def bilstm_eval(x, w_ih, w_hh, b_ih, b_hh, w_ih_r, w_hh_r, b_ih_r, b_hh_r):
    """one bidirectional LSTM layer, batch-first (N, T, C) -> (N, T, 2 Hh), zero initial state, evaluation only: the input
    projections of both directions as two linear launches, then per time step the split-K recurrent GEMM + the gate kernel of the
    text-prior generator (csrc/crnn.hip)"""
    _chk(x, w_ih, w_hh, b_ih, b_hh, w_ih_r, w_hh_r, b_ih_r, b_hh_r)
    if x.requires_grad:
        raise RuntimeError("bilstm_eval is an evaluation path (no gradient)")
    with torch.no_grad():
        N, T, Cin = x.shape
        Hh = w_hh.shape[1]
        G4 = 4 * Hh
        xf = _c(x).reshape(N * T, Cin)
        G = cat([PackedLinear(w_ih, b_ih)(xf).reshape(N, 1, T, G4), PackedLinear(w_ih_r, b_ih_r)(xf).reshape(N, 1, T, G4)])   # [N][T][2][4Hh]
        whh = _new(x, 2, Hh, G4)
        bhh = _new(x, 2, G4)
        for d, (w, b) in enumerate(((w_hh, b_hh), (w_hh_r, b_hh_r))):
            K.pack_conv_weight(_c(w.detach()).reshape(G4, Hh, 1, 1), G4, Hh, 1, 1, whh[d], None)
            K.copy(_c(b.detach()), bhh[d], G4)
        S = max(1, Hh // 32)
        gh = _new(x, S, 2, N, G4)
        Cst, out = _new(x, N, T, 2, Hh), _new(x, N, T, 2 * Hh)
        for s in range(T):
            if s > 0:
                a = [out.data_ptr() + 4 * ((s - 1 if d == 0 else T - s) * 2 * Hh + d * Hh) for d in range(2)]
                K.lstm_rec_gemm(a[0], a[1], T * 2 * Hh, whh[0], whh[1], N, Hh, G4, S, gh)
            K.lstm_step_fwd(G, gh if s > 0 else None, S, bhh, Cst, out, N, T, Hh, s)
        return out


# ---- evaluation-only helpers of the MORAN recognizer (model/moran/*) -------------------------------------------------------
def signed_relu_pool_diff(x, kernel, stride):
    """max_pool(relu(x)) - max_pool(relu(-x)) (morn.py:61-63), x NHWC, no autograd: two fused scale-activation-pool launches and a
    subtraction"""
    _chk(x)
    x = _c(x)
    N, H, W, C = x.shape
    k = (kernel, kernel) if isinstance(kernel, int) else tuple(kernel)
    s = (stride, stride) if isinstance(stride, int) else tuple(stride)
    OH, OW = (H - k[0]) // s[0] + 1, (W - k[1]) // s[1] + 1
    pos, neg = _new(x, N, OH, OW, C), _new(x, N, OH, OW, C)
    minus, zero = torch.full((C,), -1.0, dtype=F32, device=x.device), torch.zeros(C, dtype=F32, device=x.device)
    K.pool2d_fwd(x, N, H, W, C, None, None, "relu", k, s, (0, 0), pos)
    K.pool2d_fwd(x, N, H, W, C, minus, zero, "relu", k, s, (0, 0), neg)
    K.scale_(neg, neg.numel(), minus[:1])
    out = torch.empty_like(pos)
    K.add(pos, neg, pos.numel(), out)
    return out


def offset_grid_y(grid, dy):
    """sampling grid (N, H, W, 2) of (x, y) with dy (N, H, W, 1) added to its y coordinates (morn.py:66-67), no autograd"""
    _chk(grid, dy)
    grid, dy = _c(grid), _c(dy)
    out = torch.empty_like(grid)
    M = grid.numel() // 2
    K.copy(grid, out, grid.numel())
    K.copy_strided(dy, 1, 0, out, 2, 1, M, 1, accumulate=True)
    return out
