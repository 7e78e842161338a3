"""The convolution / BatchNorm sections of tpgsr_amd/engine.py, one section at a time: the harness shared by tests/test_engine_conv_bn_gpu.py
and tests/test_engine_conv_bn_cpu.py.  Engine, run modes, launch log, guard, policies, limits, generators and the error measure are those of
tests/engine_layer_common.py and tests/engine_crnn_layer_common.py (imported, not restated).

`OneLayerEngine(holder, build)`: build(engine) returns a dict of the engine's own ConvLayer / BNLayer / _FC1AsConv objects over the holder's
parameters and buffers; fn(engine, layers) calls their methods and the few direct K.* launches the engine makes between them, in the order
of the TSRNEngine lines named below.  Operand packs, argument blocks, branch choices, slab reduces and arena writes are the engine's.  Every
output and workspace buffer is pre-filled with NaN, every holder ends with the `_Guard` child, `arena_untouched` is asserted.

Sections (C = 64 as the reference; one trunk case at C = 128):
  1 trunk    conv1 -> bn1 -> mish -> conv2 -> bn2 (bn2 with pad_to = C + 32)      TSRNEngine._record_fwd (the residual block's first five
             launches) and _record_bwd (bn2.backward .. conv1.dgrad); the upstream gradient is a seeded tensor (bn2.backward unfused) or the
             data gradient of a 1 x 1 ConvLayer over 192 columns with bnb = bn2.fuse_stats(...) (the position of gru1's projection)
  2 up       conv7 + bn7 -> up.fwd(in2 = b1, out_ps) -> mish -> tail.fwd -> tail_shiftsum_tanh, and back from a seeded d sr
  3 block1   9 x 9 conv 4 -> 64 (need_dgrad = False) + PReLU, back from two incoming gradients
  4 stn      the STN head down to the control points (six conv + BN + ReLU (+ pool) stages, _FC1AsConv, bnf, fc2 with wscale = 0.1), N = 5
The float64 references are stock PyTorch on the CPU with autograd: F.conv2d, F.batch_norm(training=True), F.mish, F.pixel_shuffle, F.prelu,
F.max_pool2d, F.linear (reference project: model/tsrn.py, model/stn_head.py).  `_autograd(dtype, k)` with k > 0 is the error model of the
fewer-term policies: the same computation with the operands of every GEMM rounded to k bf16 terms (forward, data gradient, weight gradient).

Bounds (nothing from the GPU):  per key  g * L + 4 e_ref32 + 4 * 2^-24,  e = max |got - ref64| / max |ref64|;  L = limits(policy), the value
entry for activations and data gradients, the parameter entry for parameter gradients;  g = the number of split-operand GEMMs between the
section's inputs and the key (the case's table `g`; 0 = the plain `arith` rule: saved statistics, running buffers, gradients no GEMM feeds).
A convolution bias in front of a training-mode BatchNorm has an analytically zero gradient: the keys of `zero_bias` are normalised per
column by the float64 sum of |dy| over the summed column instead of max |ref| -- for the GPU, for e_ref32 and for the model alike.
Under x2 / bf16 the keys a test lists (`model_keys`) add MODEL_MARGIN x the error of the float64 section on k-term GEMM operands."""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from engine_crnn_layer_common import (F64, FLOOR, GUARD, MODEL_MARGIN, MODES, POLICIES, TERMS, OneLayerEngine, _bf_terms, _gen,  # noqa: E402,F401
                                      _Guard, _pack_names, arena_untouched, conv_prec, err, launch_log, limits, run_engine)

F32 = torch.float32
EPS, MOMENTUM = 1e-5, 0.1
GP = 192                 # gate columns of the projection behind bn2 (gru1 at hidden 32: 6 x 32)
PAD = 32                 # bn2's pad_to = C + 32: the text strip's channels
NAN = float("nan")
SIZE_LIMIT = 8 << 20
SIDE_NAMES = ("tpgsr_conv_wgrad", "tpgsr_wgrad_reduce", "tpgsr_reduce_partials", "tpgsr_wgrad_reduce_program")   # recorded on the side stream
W_EAGER = ["tpgsr_conv_wgrad", "tpgsr_wgrad_reduce"]
BNB = ["tpgsr_bn_bwd_finalize", "tpgsr_bn_bwd_apply"]


# ---- float64 / float32 / k-term reference pieces ------------------------------------------------------------------------------------
class _RConv(torch.autograd.Function):
    """F.conv2d, its data gradient and its weight gradient, each on operands rounded to k bf16 terms"""

    @staticmethod
    def forward(ctx, x, w, k, pad):
        ctx.save_for_backward(x, w)
        ctx.k, ctx.pad = k, pad
        return F.conv2d(_bf_terms(x, k), _bf_terms(w, k), padding=pad)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dyr = _bf_terms(dy, ctx.k)
        return (torch.nn.grad.conv2d_input(x.shape, _bf_terms(w, ctx.k), dyr, padding=ctx.pad),
                torch.nn.grad.conv2d_weight(_bf_terms(x, ctx.k), w.shape, dyr, padding=ctx.pad), None, None)


def conv(x, w, b, pad, k=0):
    y = F.conv2d(x, w, None, padding=pad) if not k else _RConv.apply(x, w, k, pad)
    return y if b is None else y + b.view(1, -1, 1, 1)


def bnorm(y, p, pre, stats):
    """training-mode BatchNorm over dim 1 with the running buffers stats[pre + '.running_mean' / '.running_var'] updated in place"""
    return F.batch_norm(y, stats[pre + ".running_mean"], stats[pre + ".running_var"], p[pre + ".weight"], p[pre + ".bias"], training=True,
                        momentum=MOMENTUM, eps=EPS)


def saved_stats(y):
    """(mean, 1 / sqrt(biased variance + eps)) over all but dim 1"""
    dims = [d for d in range(y.dim()) if d != 1]
    return y.mean(dims), 1.0 / torch.sqrt(y.var(dims, unbiased=False) + EPS)


def to_nchw(t, N, H, W):
    return t.reshape(N, H, W, -1).permute(0, 3, 1, 2)


def to_flat(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _uniform(g, shape, bound):
    return (torch.rand(*shape, generator=g) * 2 - 1) * bound


def conv_params(g, name, cout, cin, kh, kw):
    """PyTorch's default scale: U(+-1 / sqrt(fan_in)) for weight and bias"""
    b = 1.0 / (cin * kh * kw) ** 0.5
    return {name + ".weight": _uniform(g, (cout, cin, kh, kw), b), name + ".bias": _uniform(g, (cout,), b)}


def bn_params(g, name, c):
    """gamma in [0.5, 1.5]; running buffers away from (0, 1), so an update that ignored the old value would show"""
    p = {name + ".weight": torch.rand(c, generator=g) + 0.5, name + ".bias": torch.randn(c, generator=g) * 0.5}
    b = {name + ".running_mean": torch.randn(c, generator=g) * 0.5, name + ".running_var": torch.rand(c, generator=g) + 0.5}
    return p, b


def fill_holder(m, params, buffers):
    with torch.no_grad():
        have = dict(m.named_parameters())
        assert set(have) == set(params) | {GUARD}, sorted(set(have) ^ set(params))
        for k, v in params.items():
            assert have[k].shape == v.shape, (k, tuple(have[k].shape), tuple(v.shape))
            have[k].copy_(v)
        hb = dict(m.named_buffers())
        for k, v in buffers.items():
            hb[k].copy_(v)
    return m


def nan(device, *s):
    return torch.full(s, NAN, device=device)


def nan_bn(bn, ws):
    """bind the layer's per-plan tensors and fill what a finalize has to write: scale / shift of its own channels (the identity tail
    beyond them is part of what is tested), the saved statistics and the backward coefficients"""
    bn.use(ws)
    bn.scale[:bn.C] = NAN
    bn.shift[:bn.C] = NAN
    for t in (bn.save_mean, bn.save_rstd, bn.coef):
        t.fill_(NAN)


def nan_scratch(eng, convs, bns):
    """the stream-ordered scratch of an eager run, sized as the layers size it, filled with NaN: statistics rows, weight-gradient slabs"""
    from tpgsr_amd import kernels as K
    for bn, M in bns:
        n = (M + 63) // 64 * 2 * bn.C
        for name in ("bn_partial", "bnb_partial"):
            eng.scratch(name, n)
    npart = ndb = 1
    for L, N, H, W in convs:
        g = L.geom(N, H, W)
        Z = K.wgrad_splits(g.M, g.K, g.Cout, geom=g)
        npart, ndb = max(npart, Z * g.K * g.Cout), max(ndb, Z * g.Cout)
    eng.scratch("wgrad_part", npart)
    eng.scratch("wgrad_dbpart", ndb)
    for t in eng._scratch.values():
        t.fill_(NAN)


class _Case:
    """g: key -> number of GEMMs; values: the keys bounded by the value entry of limits(); zero_bias: key -> the reference's entry holding
    the float64 sum of |dy| per summed column"""
    g, values, zero_bias = {}, (), {}

    def __init__(self):
        self._refs = {}

    @property
    def keys(self):
        return tuple(self.g)

    def computed(self, dtype=F64, k=0):
        """the section in `dtype` on k-term GEMM operands (0: exact): computed once, shared, never modified"""
        if (dtype, k) not in self._refs:
            self._refs[(dtype, k)] = {n: v.detach() for n, v in self._autograd(dtype, k).items()}
        return self._refs[(dtype, k)]

    def reference(self):
        return self.computed(F64)

    def ref32(self):
        return self.computed(F32)

    def key_err(self, key, got):
        ref = self.reference()
        if key in self.zero_bias:
            den = ref[self.zero_bias[key]]                 # (a column whose every dy is zero -- a ReLU shut for the whole batch -- has no
            return ((got.to(F64) - ref[key]).abs() / torch.where(den > 0, den, den.max())).max().item()      # scale of its own: the key's largest)
        return err(got, ref[key])

    def e_ref32(self, key):
        return self.key_err(key, self.ref32()[key])

    def model_term(self, key, policy):
        """MODEL_MARGIN x e(the float64 section on the policy's k-term GEMM operands, the float64 reference); 0 under x3 / f32"""
        k = TERMS[policy]
        return MODEL_MARGIN * self.key_err(key, self.computed(F64, k)[key]) if k in (1, 2) else 0.0

    def bound(self, key, policy, model_keys=()):
        lim = limits(policy)
        b = self.g[key] * (lim[0] if key in self.values else lim[1]) + 4 * self.e_ref32(key) + FLOOR
        if key in model_keys:
            b += self.model_term(key, policy)
        return b

    def input_bytes(self):
        return max(v.numel() * v.element_size() for v in list(self.ins.values()) + list(self.params.values()))

    def expected_launches(self, policy, mode="eager"):
        s = self.sections(policy, mode)
        return _pack_names(policy) + s["fwd"] + s["bwd"] + (["tpgsr_wgrad_reduce_program"] if mode == "recorded" else [])

    def _w(self, mode):
        return ["tpgsr_conv_wgrad"] if mode == "recorded" else list(W_EAGER)

    def _grads(self, eng, got):
        for k, v in self.params.items():
            if k in self.g:
                got[k] = eng.G[k].detach().cpu().view(v.shape).clone()
        arena_untouched(eng, [k for k in self.params if k in self.g])


# ---- 1: the trunk pair ---------------------------------------------------------------------------------------------------------------
TRUNK_MAPS = [(2, 16, 64), (1, 16, 64), (3, 5, 7)]      # M = 2048, 1024, 105 (a ragged last statistics block; tiles that fit neither 16 rows nor 64 columns)
TRUNK_VARIANTS = ("seeded", "proj")
STAT_KEYS = tuple(f"{b}.{s}" for b in ("bn1", "bn2") for s in ("save_mean", "save_rstd"))
RUN_KEYS = tuple(f"{b}.running_{s}" for b in ("bn1", "bn2") for s in ("mean", "var"))


class TrunkCase(_Case):
    values = ("y1", "y2", "out", "dx")

    def __init__(self, C, N, H, W, variant):
        super().__init__()
        self.C, self.N, self.H, self.W, self.variant = C, N, H, W, variant
        self.M = M = N * H * W
        self.id = f"trunk-C{C}-{N}x{H}x{W}-{variant}"
        g = _gen("engine-trunk", C, N, H, W)                 # (both variants share the forward pass)
        self.params, self.buffers = {}, {}
        self.params.update(conv_params(g, "c1", C, C, 3, 3))
        for n in ("bn1", "bn2"):
            p, b = bn_params(g, n, C)
            if n == "bn2":
                self.params.update(conv_params(g, "c2", C, C, 3, 3))
            self.params.update(p)
            self.buffers.update(b)
        self.ins = {"x": torch.randn(M, C, generator=g)}
        gu = _gen("engine-trunk-upstream", self.id)
        p = int(variant == "proj")
        if p:
            self.params.update(conv_params(gu, "proj", GP, C, 1, 1))
            self.ins["dgi"] = torch.randn(M, GP, generator=gu)
        else:
            self.ins["da"] = torch.randn(M, C, generator=gu)
        # GEMMs between the inputs and the key: the forward convolutions before it, then (+ p: the projection's data gradient) the data /
        # weight gradients on the way back
        self.g = {"y1": 1, "y2": 2, "out": 2, "dx": 4 + p, "c2.weight": 3 + p, "c2.bias": 2 + p, "bn2.weight": 2 + p, "bn2.bias": 2 + p,
                  "c1.weight": 4 + p, "c1.bias": 3 + p, "bn1.weight": 3 + p, "bn1.bias": 3 + p}
        self.g.update({k: 0 for k in STAT_KEYS})
        self.g.update({f"{k}@{n}": 0 for k in RUN_KEYS for n in (1, 2)})
        self.zero_bias = {"c1.bias": "_sum|dy|1", "c2.bias": "_sum|dy|2"}

    def _autograd(self, dtype, k=0, mutate=None):
        N, H, W = self.N, self.H, self.W
        p = {n: v.to(dtype).clone().requires_grad_(True) for n, v in self.params.items()}
        st = {n: v.to(dtype).clone() for n, v in self.buffers.items()}
        x = to_nchw(self.ins["x"].to(dtype), N, H, W).clone().requires_grad_(True)
        out = {}
        for n in (1, 2):                                       # two forward passes over the same input: the running buffers move twice
            y1 = conv(x, p["c1.weight"], p["c1.bias"], 1, k)
            a1 = F.mish(bnorm(y1, p, "bn1", st))
            y2 = conv(a1, p["c2.weight"], p["c2.bias"], 1, k)
            z2 = bnorm(y2, p, "bn2", st)
            out.update({f"{key}@{n}": st[key].clone() for key in RUN_KEYS})
        y1.retain_grad()
        y2.retain_grad()
        if self.variant == "proj":
            da = to_nchw(self.ins["dgi"].to(dtype), N, H, W)
            da = conv(da, p["proj.weight"].detach().permute(1, 0, 2, 3), None, 0, k)       # dgi W: the 1 x 1 convolution's data gradient
        else:
            da = to_nchw(self.ins["da"].to(dtype), N, H, W)
        (z2 * da.detach()).sum().backward()
        out.update({"y1": to_flat(y1), "y2": to_flat(y2), "out": to_flat(z2), "dx": to_flat(x.grad)})
        for b, y in (("bn1", y1), ("bn2", y2)):
            out[b + ".save_mean"], out[b + ".save_rstd"] = saved_stats(y)
        out.update({n: p[n].grad for n in self.g if n in p})
        out["_sum|dy|1"], out["_sum|dy|2"] = to_flat(y1.grad).abs().sum(0), to_flat(y2.grad).abs().sum(0)
        if mutate == "rm_without_bias":                         # the conv bias left out of the running mean's update
            for n in (1, 2):
                prev = self.buffers["bn1.running_mean"].to(dtype)
                for _ in range(n):
                    prev = (1 - MOMENTUM) * prev + MOMENTUM * (out["bn1.save_mean"] - p["c1.bias"].detach())
                out[f"bn1.running_mean@{n}"] = prev
        if mutate == "stat_tail_dropped":                       # the last M % 64 rows' contribution to the BatchNorm sums dropped
            y = to_flat(y1.detach()).clone()
            y[self.M // 64 * 64:] = 0
            mean = y.sum(0) / self.M
            var = (y * y).sum(0) / self.M - mean * mean
            out["bn1.save_mean"], out["bn1.save_rstd"] = mean, 1.0 / torch.sqrt(var.clamp_min(0) + EPS)
        return out

    def fused(self, policy):
        """(bn2's, bn1's backward sums ride on the producing data gradient)"""
        split = bool(TERMS[policy])
        return split and self.variant == "proj", split

    def sections(self, policy, mode="eager", fwd_passes=None):
        passes = (2 if mode == "recorded" else 1) if fwd_passes is None else fwd_passes
        f2, f1 = self.fused(policy)
        red = lambda fused: [] if fused else ["tpgsr_bn_bwd_reduce"]
        w = self._w(mode)
        fwd = ["tpgsr_conv_fwd", "tpgsr_bn_finalize", "tpgsr_affine_act", "tpgsr_conv_fwd", "tpgsr_bn_finalize"] * passes + ["tpgsr_affine_act"]
        bwd = (["tpgsr_conv_fwd"] if self.variant == "proj" else []) + red(f2) + BNB + w + ["tpgsr_conv_fwd"] + red(f1) + BNB + w + ["tpgsr_conv_fwd"]
        return dict(fwd=fwd, bwd=bwd)


def trunk_cases():
    return [TrunkCase(64, *m, v) for m in TRUNK_MAPS for v in TRUNK_VARIANTS] + [TrunkCase(128, 3, 5, 7, "proj")]      # + the `hd_u 64` width


def trunk_holder(case):
    from tpgsr_amd.model import nn_params as P

    class Holder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            C = case.C
            self.c1, self.bn1 = P.Conv2dParams(C, C, 3, padding=1), P.BatchNormParams(C)
            self.c2, self.bn2 = P.Conv2dParams(C, C, 3, padding=1), P.BatchNormParams(C)
            if case.variant == "proj":
                self.proj = P.Conv2dParams(C, GP, 1)
            self.end = _Guard(4 * 9 * C)
    return fill_holder(Holder(), case.params, case.buffers)


def run_trunk(case, device, mode="eager"):
    """-> (every key of the case on the CPU, the launches, what the run saw: branches, row granularities, the identity tail).
    eager: one forward pass; recorded: two (the running buffers move twice: the `@2` keys), then one backward pass"""
    from tpgsr_amd import engine, kernels as K

    def build(e):
        L = dict(conv1=engine.ConvLayer(e, "c1.weight", "c1.bias", 3, 3, 1, 1), bn1=engine.BNLayer(e, "bn1"),
                 conv2=engine.ConvLayer(e, "c2.weight", "c2.bias", 3, 3, 1, 1), bn2=engine.BNLayer(e, "bn2", pad_to=case.C + PAD))
        if case.variant == "proj":
            L["proj"] = engine.ConvLayer(e, "proj.weight", "proj.bias")
        return L
    eng = OneLayerEngine(trunk_holder(case).to(device), build)
    N, H, W, M, C = case.N, case.H, case.W, case.M, case.C
    d = {k: v.to(device).contiguous() for k, v in case.ins.items()}
    buf = {k: nan(device, M, C) for k in ("y1", "a1", "y2", "out", "da", "dy2", "da1", "dy1", "dx")}
    passes = 2 if mode == "recorded" else 1
    seen = {}

    def fn(eng, L):
        c1, c2, bn1, bn2 = L["conv1"], L["conv2"], L["bn1"], L["bn2"]
        nan_bn(bn1, eng._cur_ws)
        nan_bn(bn2, eng._cur_ws)
        nan_scratch(eng, [(c1, N, H, W), (c2, N, H, W)], [(bn1, M), (bn2, M)])
        for _ in range(passes):                                           # engine.py: TSRNEngine._record_fwd, the residual block
            part, _n = bn1.partial(M)
            g1 = c1.fwd(N, H, W, d["x"], buf["y1"], bn_partial=part, bn_coarse=True)
            bn1.finalize(M, c1.b, True, g1.bn_row_tiles)
            K.affine_act(buf["y1"], M, C, bn1.scale, bn1.shift, "mish", buf["a1"])
            g2 = c2.fwd(N, H, W, buf["a1"], buf["y2"], bn_partial=part, bn_coarse=True)
            bn2.finalize(M, c2.b, True, g2.bn_row_tiles)
        K.affine_act(buf["y2"], M, C, bn2.loader["in_scale"], bn2.loader["in_shift"], "none", buf["out"])
        seen["fwd_row_tiles"] = (g1.bn_row_tiles, g2.bn_row_tiles)
        if case.variant == "proj":                                        # TSRNEngine._record_bwd: fz2, gru1's data gradient, then the block
            fz2 = bn2.fuse_stats(buf["y2"], M, "none", L["proj"].Cout)
            L["proj"].dgrad(N, H, W, d["dgi"], buf["da"], bnb=fz2)
            da = buf["da"]
        else:
            fz2, da = None, d["da"]
        bn2.backward(da, None, buf["y2"], M, "none", buf["dy2"], fused=fz2)
        c2.wgrad(N, H, W, buf["a1"], buf["dy2"])
        fz1 = bn1.fuse_stats(buf["y1"], M, "mish", c2.Cout)
        c2.dgrad(N, H, W, buf["dy2"], buf["da1"], bnb=fz1)
        bn1.backward(buf["da1"], None, buf["y1"], M, "mish", buf["dy1"], fused=fz1)
        c1.wgrad(N, H, W, d["x"], buf["dy1"])
        c1.dgrad(N, H, W, buf["dy1"], buf["dx"])
        seen["fused"] = (fz2 is not None, fz1 is not None)
        seen["bwd_row_tiles"] = tuple(None if fz is None else fz["row_tiles"] for fz in (fz2, fz1))

    with launch_log() as names:
        run_engine(eng, fn, device, mode)
    L = eng.layer
    got = {k: buf[k].cpu() for k in ("y1", "y2", "out", "dx")}
    for b in ("bn1", "bn2"):
        got[b + ".save_mean"], got[b + ".save_rstd"] = L[b].save_mean.cpu(), L[b].save_rstd.cpu()
        for s in ("running_mean", "running_var"):
            got[f"{b}.{s}@{passes}"] = eng.B[f"{b}.{s}"].detach().cpu().clone()
    seen["tail"] = (L["bn2"].scale.cpu()[C:].clone(), L["bn2"].shift.cpu()[C:].clone())
    seen["bn1_len"] = L["bn1"].scale.numel()
    case._grads(eng, got)
    return got, names, seen


def run_bn_eval(case, device):
    """BNLayer.finalize(training=False) over the case's bn2: (scale, shift, the running buffers afterwards) and the launches"""
    from tpgsr_amd import engine
    eng = OneLayerEngine(trunk_holder(case).to(device), lambda e: dict(bn2=engine.BNLayer(e, "bn2", pad_to=case.C + PAD)))

    def fn(eng, L):
        nan_bn(L["bn2"], eng._cur_ws)
        L["bn2"].finalize(case.M, None, False)
    with launch_log() as names:
        eng.run(fn, device)
    bn = eng.layer["bn2"]
    arena_untouched(eng, [])
    return dict(scale=bn.scale.cpu(), shift=bn.shift.cpu(), rm=eng.B["bn2.running_mean"].cpu(), rv=eng.B["bn2.running_var"].cpu()), names


# ---- 2: block 7 + upsample block + tail ----------------------------------------------------------------------------------------------
UP_MAPS = [(2, 16, 64), (1, 5, 7)]
CO, KS = 4, 9


def pixel_shuffle(u, mutate=None):
    if mutate == "ps_phase":                                    # the two phase bits swapped: channel c*4 + i*2 + j lands at (2w + i, 2h + j)
        n, c4, h, w = u.shape
        u = u.view(n, c4 // 4, 2, 2, h, w).transpose(2, 3).reshape(n, c4, h, w)
    return F.pixel_shuffle(u, 2)


class UpCase(_Case):
    values = ("sr", "dcur", "db1")
    g = {"sr": 3, "tail.weight": 4, "tail.bias": 3, "up.weight": 5, "up.bias": 4, "db1": 5, "bn7.weight": 5, "bn7.bias": 5, "c7.bias": 5,
         "c7.weight": 6, "dcur": 6}
    zero_bias = {"c7.bias": "_sum|dy|7"}

    def __init__(self, N, H, W, C=64):
        super().__init__()
        self.C, self.N, self.H, self.W = C, N, H, W
        self.M = M = N * H * W
        self.id = f"up-C{C}-{N}x{H}x{W}"
        g = _gen("engine-up", self.id)
        self.params = conv_params(g, "c7", C, C, 3, 3)
        p, self.buffers = bn_params(g, "bn7", C)
        self.params.update(p)
        self.params.update(conv_params(g, "up", 4 * C, C, 3, 3))
        self.params.update(conv_params(g, "tail", CO, C, KS, KS))
        self.ins = {"cur": torch.randn(M, C, generator=g), "b1": torch.randn(M, C, generator=g),
                    "dsr": torch.randn(N, CO, 2 * H, 2 * W, generator=g)}

    def _autograd(self, dtype, k=0, mutate=None):
        N, H, W = self.N, self.H, self.W
        p = {n: v.to(dtype).clone().requires_grad_(True) for n, v in self.params.items()}
        st = {n: v.to(dtype).clone() for n, v in self.buffers.items()}
        cur = to_nchw(self.ins["cur"].to(dtype), N, H, W).clone().requires_grad_(True)
        b1 = to_nchw(self.ins["b1"].to(dtype), N, H, W).clone().requires_grad_(True)
        y7 = conv(cur, p["c7.weight"], p["c7.bias"], 1, k)
        y7.retain_grad()
        u = conv(bnorm(y7, p, "bn7", st) + b1, p["up.weight"], p["up.bias"], 1, k)
        mu = F.mish(pixel_shuffle(u, mutate))
        sr = torch.tanh(conv(mu, p["tail.weight"], p["tail.bias"], KS // 2, k))
        (sr * self.ins["dsr"].to(dtype)).sum().backward()
        out = {"sr": sr, "dcur": to_flat(cur.grad), "db1": to_flat(b1.grad), "_sum|dy|7": to_flat(y7.grad).abs().sum(0)}
        out.update({n: p[n].grad for n in p})
        return out

    def sections(self, policy, mode="eager"):
        split = bool(TERMS[policy])
        w = self._w(mode)
        fwd = ["tpgsr_conv_fwd", "tpgsr_bn_finalize", "tpgsr_conv_fwd", "tpgsr_affine_act", "tpgsr_conv_fwd", "tpgsr_tail_shiftsum_tanh"]
        bwd = ["tpgsr_tail_bwd", "tpgsr_reduce_partials"] + w + ["tpgsr_conv_fwd"] + ([] if split else ["tpgsr_act_bwd"]) + w + ["tpgsr_conv_fwd"] \
            + ([] if split else ["tpgsr_bn_bwd_reduce"]) + BNB + w + ["tpgsr_conv_fwd"]
        return dict(fwd=fwd, bwd=bwd)


def up_cases():
    return [UpCase(*m) for m in UP_MAPS]


def up_holder(case):
    from tpgsr_amd.model import nn_params as P

    class Holder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            C = case.C
            self.c7, self.bn7 = P.Conv2dParams(C, C, 3, padding=1), P.BatchNormParams(C)
            self.up = P.Conv2dParams(C, 4 * C, 3, padding=1)
            self.tail = P.Conv2dParams(C, CO, KS, padding=KS // 2)
            self.end = _Guard(4 * 9 * C)
    return fill_holder(Holder(), case.params, case.buffers)


def run_up(case, device, mode="eager"):
    from tpgsr_amd import engine, kernels as K
    build = lambda e: dict(conv7=engine.ConvLayer(e, "c7.weight", "c7.bias", 3, 3, 1, 1), bn7=engine.BNLayer(e, "bn7"),
                           up=engine.ConvLayer(e, "up.weight", "up.bias", 3, 3, 1, 1), tail=engine.ConvLayer(e, "tail.weight", None, tail=True))
    eng = OneLayerEngine(up_holder(case).to(device), build)
    N, H, W, M, C = case.N, case.H, case.W, case.M, case.C
    H2, W2, P4 = 2 * H, 2 * W, 4 * M
    d = {k: v.to(device).contiguous() for k, v in case.ins.items()}
    buf = {k: nan(device, M, C) for k in ("y7", "d_s", "dy", "gA")}
    buf.update({k: nan(device, P4, C) for k in ("ups", "mups", "d_ups")})
    buf.update(Pt=nan(device, P4, KS * CO), dPt=nan(device, P4, KS * CO), sr=nan(device, N, CO, H2, W2))
    seen = {}

    def fn(eng, L):
        c7, bn7, up, tl = L["conv7"], L["bn7"], L["up"], L["tail"]
        assert (tl.Cout, tl.Co, tl.KS, tl.KH, tl.KW, tl.pad_h) == (KS * CO, CO, KS, KS, 1, KS // 2)
        nan_bn(bn7, eng._cur_ws)
        nan_scratch(eng, [(c7, N, H, W), (up, N, H, W), (tl, N, H2, W2)], [(bn7, M)])
        part, _n = bn7.partial(M)                                          # TSRNEngine._record_fwd: block 7 .. sr
        g7 = c7.fwd(N, H, W, d["cur"], buf["y7"], bn_partial=part, bn_coarse=True)
        bn7.finalize(M, c7.b, True, g7.bn_row_tiles)
        up.fwd(N, H, W, buf["y7"], buf["ups"], in2=d["b1"], out_ps=True, **bn7.loader)
        K.affine_act(buf["ups"], P4, C, None, None, "mish", buf["mups"])
        tl.fwd(N, H2, W2, buf["mups"], buf["Pt"])
        K.tail_shiftsum_tanh(buf["Pt"], eng.P["tail.bias"], N, H2, W2, tl.Co, tl.KS, buf["sr"])
        nblk = K.tail_bwd_blocks(N, H2, W2, tl.Co, tl.KS)                   # TSRNEngine._record_bwd: the tail .. conv7.dgrad
        dbp = eng.scratch("tail_dbp", nblk * tl.Co)
        dbp.fill_(NAN)
        K.tail_bwd(buf["sr"], d["dsr"], N, H2, W2, tl.Co, tl.KS, buf["dPt"], dbp, nblk)
        with K.side():
            K.reduce_partials(dbp, nblk, tl.Co, eng.G["tail.bias"], accumulate=True)
        tl.wgrad(N, H2, W2, buf["mups"], buf["dPt"])
        seen["mish_epilogue"] = K.bnb_fusable(tl.Cout)
        if seen["mish_epilogue"]:
            tl.dgrad(N, H2, W2, buf["dPt"], buf["d_ups"], bnb=dict(y=buf["ups"], act="mish", store_dz=True))
        else:
            tl.dgrad(N, H2, W2, buf["dPt"], buf["d_ups"])
            K.act_bwd(buf["ups"], buf["d_ups"], P4 * C, "mish", buf["d_ups"])
        up.wgrad(N, H, W, buf["y7"], buf["d_ups"], loader=dict(in2=d["b1"], **bn7.loader), dy_kw=dict(dy_ps=True))
        fz7 = bn7.fuse_stats(buf["y7"], M, "none", up.Cout)
        up.dgrad(N, H, W, buf["d_ups"], buf["d_s"], in_ps=True, bnb=fz7)
        bn7.backward(buf["d_s"], None, buf["y7"], M, "none", buf["dy"], fused=fz7)
        c7.wgrad(N, H, W, d["cur"], buf["dy"])
        c7.dgrad(N, H, W, buf["dy"], buf["gA"])
        seen["fused"] = fz7 is not None
        seen["row_tiles"] = (g7.bn_row_tiles, None if fz7 is None else fz7["row_tiles"])

    with launch_log() as names:
        run_engine(eng, fn, device, mode)
    got = {"sr": buf["sr"].cpu(), "dcur": buf["gA"].cpu(), "db1": buf["d_s"].cpu()}
    case._grads(eng, got)
    return got, names, seen


# ---- 3: block1 + PReLU ---------------------------------------------------------------------------------------------------------------
B1_MAPS = [(2, 16, 64), (3, 5, 7)]
B1_SEEDS = tuple(range(401, 417))
CI = 4
PRELU_BLOCKS = 1024


class Block1Case(_Case):
    """Conv2d(4, 64, 9, padding=4) -> PReLU (one slope).  The first seed of B1_SEEDS that keeps every float64 and float32 c1 further from the
    PReLU's kink than 8 * 2^-24 * (|w| * |x| + |b|), the scale of a float32 convolution's rounding error (which element takes the slope
    decides its whole gradient)"""
    values = ("c1", "b1")
    g = {"c1": 1, "b1": 1, "b.weight": 2, "b.bias": 1, "pr.weight": 1}

    def __init__(self, N, H, W, C=64):
        super().__init__()
        self.C, self.N, self.H, self.W = C, N, H, W
        self.M = M = N * H * W
        self.id = f"block1-{N}x{H}x{W}"
        self.buffers = {}
        self.seed = None
        for seed in B1_SEEDS:
            g = _gen("engine-block1", self.id, seed)
            self.params = conv_params(g, "b", C, CI, KS, KS)
            self.params["pr.weight"] = torch.full((1,), 0.25)
            self.ins = {"x": torch.rand(M, CI, generator=g), "gA": torch.randn(M, C, generator=g), "d_s": torch.randn(M, C, generator=g)}
            self.near = self.near_kink()
            if self.near == (0, 0):
                self.seed = seed
                break
        assert self.seed is not None, "no seed of B1_SEEDS keeps c1 clear of the PReLU's kink"

    def near_kink(self):
        out = []
        for dtype in (F64, F32):
            x = to_nchw(self.ins["x"].to(dtype), self.N, self.H, self.W)
            w, b = self.params["b.weight"].to(dtype), self.params["b.bias"].to(dtype)
            c1, mag = F.conv2d(x, w, b, padding=KS // 2), F.conv2d(x.abs(), w.abs(), b.abs(), padding=KS // 2)
            out.append(int((c1.abs() < 8 * 2.0 ** -24 * mag).sum()))
        return tuple(out)

    def _autograd(self, dtype, k=0, mutate=None):
        N, H, W = self.N, self.H, self.W
        p = {n: v.to(dtype).clone().requires_grad_(True) for n, v in self.params.items()}
        x = to_nchw(self.ins["x"].to(dtype), N, H, W)
        c1 = conv(x, p["b.weight"], p["b.bias"], KS // 2, k)
        b1 = F.prelu(c1, p["pr.weight"])
        (b1 * to_nchw((self.ins["gA"].to(dtype) + self.ins["d_s"].to(dtype)), N, H, W)).sum().backward()
        out = {"c1": to_flat(c1), "b1": to_flat(b1)}
        out.update({n: p[n].grad for n in p})
        return out

    def sections(self, policy, mode="eager"):
        return dict(fwd=["tpgsr_conv_fwd", "tpgsr_prelu_fwd"], bwd=["tpgsr_prelu_bwd", "tpgsr_reduce_partials"] + self._w(mode))


def block1_cases():
    return [Block1Case(*m) for m in B1_MAPS]


def block1_holder(case):
    from tpgsr_amd.model import nn_params as P

    class Holder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.b, self.pr = P.Conv2dParams(CI, case.C, KS, padding=KS // 2), P.PReLUParams()
            self.end = _Guard(4 * KS * KS * CI)
    return fill_holder(Holder(), case.params, case.buffers)


def run_block1(case, device, mode="eager"):
    from tpgsr_amd import engine, kernels as K
    eng = OneLayerEngine(block1_holder(case).to(device),
                         lambda e: dict(block1=engine.ConvLayer(e, "b.weight", "b.bias", KS, KS, KS // 2, KS // 2, need_dgrad=False)))
    N, H, W, M, C = case.N, case.H, case.W, case.M, case.C
    d = {k: v.to(device).contiguous() for k, v in case.ins.items()}
    buf = {k: nan(device, M, C) for k in ("c1", "b1", "dc1")}

    def fn(eng, L):
        b = L["block1"]
        assert b.wt_d is None
        nan_scratch(eng, [(b, N, H, W)], [])
        b.fwd(N, H, W, d["x"], buf["c1"])                                   # TSRNEngine._record_fwd_pre
        K.prelu_fwd(buf["c1"], eng.P["pr.weight"], M * C, buf["b1"])
        dap = eng.scratch("prelu_dap", PRELU_BLOCKS)                        # TSRNEngine._record_bwd: b1 receives d_s + gA
        dap.fill_(NAN)
        K.prelu_bwd(buf["c1"], eng.P["pr.weight"], d["gA"], d["d_s"], M * C, buf["dc1"], dap, PRELU_BLOCKS)
        with K.side():
            K.reduce_partials(dap, PRELU_BLOCKS, 1, eng.G["pr.weight"], accumulate=True)
        b.wgrad(N, H, W, d["x"], buf["dc1"])

    with launch_log() as names:
        run_engine(eng, fn, device, mode)
    got = {"c1": buf["c1"].cpu(), "b1": buf["b1"].cpu()}
    case._grads(eng, got)
    return got, names, {}


# ---- 4: the STN head down to the control points --------------------------------------------------------------------------------------
STN_N, STN_H, STN_W, NCTRL = 5, 16, 64, 20       # (N = 2 would make every BatchNorm's input gradient identically zero)
STN_CH = [(CI, 32), (32, 64), (64, 128), (128, 256), (256, 256), (256, 256)]
STN_POOLS = [(2, 2), (2, 2), (2, 2), (2, 2), (1, 2), None]
STN_SEEDS = tuple(range(301, 317))
STN_SEED = 304           # the first seed of STN_SEEDS with no ReLU and no max-pool decision inside the margin (the CPU test asserts it)
CP = [f"stn_head.stn_convnet.{2 * i}" for i in range(6)]
FC1, BNF, FC2 = "stn_head.stn_fc1.0", "stn_head.stn_fc1.1", "stn_head.stn_fc2"


class StnCase(_Case):
    values = ("ctrl",)

    def __init__(self, seed=STN_SEED):
        super().__init__()
        self.N, self.seed = STN_N, seed
        self.id = f"stn-{STN_N}x{STN_H}x{STN_W}-seed{seed}"
        g = _gen("engine-stn", seed)
        self.params, self.buffers = {}, {}
        for i, (ci, co) in enumerate(STN_CH):
            self.params.update(conv_params(g, CP[i] + ".0", co, ci, 3, 3))
            p, b = bn_params(g, CP[i] + ".1", co)
            self.params.update(p)
            self.buffers.update(b)
        lin = lambda name, co, ci: {name + ".weight": _uniform(g, (co, ci), ci ** -0.5), name + ".bias": _uniform(g, (co,), ci ** -0.5)}
        self.params.update(lin(FC1, 512, 512))
        p, b = bn_params(g, BNF, 512)
        self.params.update(p)
        self.buffers.update(b)
        self.params.update(lin(FC2, 2 * NCTRL, 512))
        self.ins = {"x": torch.rand(STN_N * STN_H * STN_W, CI, generator=g), "dctrl": torch.randn(STN_N, 2 * NCTRL, generator=g)}
        # GEMMs: six convolutions, fc1, fc2 forward; back: fc2's data gradient (bnf's backward reads f1: the seven forward ones), fc1's,
        # then one data gradient per stage -- the gradient entering stage i has seen 14 - i, its weight gradient is one more
        self.g = {"ctrl": 8, FC2 + ".weight": 8, FC2 + ".bias": 0, BNF + ".weight": 8, BNF + ".bias": 8, FC1 + ".bias": 8, FC1 + ".weight": 9}
        self.zero_bias = {FC1 + ".bias": "_sum|dy|f"}
        for i in range(6):
            self.g.update({CP[i] + ".0.weight": 15 - i, CP[i] + ".0.bias": 14 - i, CP[i] + ".1.weight": 14 - i, CP[i] + ".1.bias": 14 - i})
            self.zero_bias[CP[i] + ".0.bias"] = f"_sum|dy|{i}"
        self.Ms = [STN_N * h * w for h, w in ((16, 64), (8, 32), (4, 16), (2, 8), (1, 4), (1, 2))] + [STN_N]

    def _autograd(self, dtype, k=0, mutate=None, decisions=None):
        """decisions (a list): gets, per stage, (ReLU pre-activations inside the margin, pool windows whose two largest lie inside it, elements)"""
        N = self.N
        p = {n: v.to(dtype).clone().requires_grad_(True) for n, v in self.params.items()}
        st = {n: v.to(dtype).clone() for n, v in self.buffers.items()}
        h = to_nchw(self.ins["x"].to(dtype), N, STN_H, STN_W)
        ys = []
        for i, pool in enumerate(STN_POOLS):                     # model/stn_head.py: Conv2d, BatchNorm2d, ReLU, MaxPool2d
            y = conv(h, p[CP[i] + ".0.weight"], p[CP[i] + ".0.bias"], 1, k)
            y.retain_grad()
            ys.append(y)
            z = bnorm(y, p, CP[i] + ".1", st)
            if decisions is not None:
                decisions.append(_decisions(y.detach(), z.detach(), p[CP[i] + ".1.bias"].detach(), pool))
            h = torch.relu(z)
            if pool is not None:
                h = F.max_pool2d(h, pool, pool)
        w1 = p[FC1 + ".weight"]
        if mutate == "fc1_taps":                                 # the two w taps of the NCHW flatten (c * 2 + w) swapped
            w1 = w1.view(512, 256, 2).flip(2).reshape(512, 512)
        f1 = conv(h.reshape(N, 512, 1, 1), w1.view(512, 512, 1, 1), p[FC1 + ".bias"], 0, k)
        f1.retain_grad()
        zf = bnorm(f1, p, BNF, st)
        if decisions is not None:
            decisions.append(_decisions(f1.detach(), zf.detach(), p[BNF + ".bias"].detach(), None))
        feat = torch.relu(zf)
        ctrl = conv(0.1 * feat, p[FC2 + ".weight"].view(2 * NCTRL, 512, 1, 1), p[FC2 + ".bias"], 0, k).reshape(N, 2 * NCTRL)
        (ctrl * self.ins["dctrl"].to(dtype)).sum().backward()
        out = {"ctrl": ctrl}
        out.update({n: p[n].grad for n in p})
        for i, y in enumerate(ys):
            out[f"_sum|dy|{i}"] = to_flat(y.grad).abs().sum(0)
        out["_sum|dy|f"] = to_flat(f1.grad).abs().sum(0)
        if mutate == "fc2_scale":                                # fc2's 0.1 dropped from its weight gradient (gscale of the slab reduce)
            out[FC2 + ".weight"] = out[FC2 + ".weight"] / 0.1
        return out

    def decisions(self, dtype):
        d = []
        self._autograd(dtype, 0, decisions=d)
        return d

    def sections(self, policy, mode="eager"):
        w = self._w(mode)
        bnb = ["tpgsr_bn_bwd_reduce"] + BNB                       # the STN head's BatchNorms keep their own statistics launch
        fwd = ["tpgsr_conv_fwd", "tpgsr_bn_finalize", "tpgsr_affine_act_pool"] * 5 + ["tpgsr_conv_fwd", "tpgsr_bn_finalize"] * 2 + ["tpgsr_conv_fwd"]
        bwd = w + ["tpgsr_conv_fwd"] + bnb + w + ["tpgsr_conv_fwd"] + bnb + w + ["tpgsr_conv_fwd"]
        for i in range(4, -1, -1):
            bwd += ["tpgsr_affine_act_pool_bwd"] + bnb + w + (["tpgsr_conv_fwd"] if i else [])
        return dict(fwd=fwd, bwd=bwd)


def _decisions(y, z, beta, pool):
    """z = scale * y + shift is the ReLU's pre-activation; the margin of an element is 8 * 2^-24 * (|scale * y| + |shift|) = 8 * 2^-24 * (|z - shift| + |shift|)
    with shift = beta - mean * scale, recovered per channel from z and y"""
    dims = [d for d in range(y.dim()) if d != 1]
    ym, zm = y.mean(dims, keepdim=True), z.mean(dims, keepdim=True)
    scale = ((z - zm) * (y - ym)).sum(dims, keepdim=True) / ((y - ym) ** 2).sum(dims, keepdim=True)
    shift = zm - scale * ym
    margin = 8 * 2.0 ** -24 * ((scale * y).abs() + shift.abs())
    relu = int((z.abs() < margin).sum())
    pools = 0
    if pool is not None and pool != (1, 1):
        n, c, h, w = z.shape
        ph, pw = pool
        win = lambda t: t.view(n, c, h // ph, ph, w // pw, pw).permute(0, 1, 2, 4, 3, 5).reshape(n, c, h // ph, w // pw, ph * pw)
        r, m = win(torch.relu(z)), win(margin)
        top, idx = r.topk(2, dim=-1)
        tie = (top[..., 0] > 0) & ((top[..., 0] - top[..., 1]) < torch.maximum(m.gather(-1, idx[..., :1]), m.gather(-1, idx[..., 1:])).squeeze(-1))
        pools = int(tie.sum())
    return relu, pools, z.numel()


def first_stn_seed():
    for seed in STN_SEEDS:
        c = StnCase(seed)
        if all(r == 0 and q == 0 for dt in (F64, F32) for r, q, _n in c.decisions(dt)):
            return seed
    return None


def stn_holder(case):
    from tpgsr_amd.model.stn_head import STNHead

    class Holder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.stn_head = STNHead(CI, NCTRL, "none", input_size=[STN_H, STN_W])
            self.end = _Guard(4 * 9 * 256)
    return fill_holder(Holder(), case.params, case.buffers)


def run_stn(case, device, mode="eager"):
    from tpgsr_amd import engine, kernels as K
    pools = engine.TSRNEngine.STN_POOLS

    def build(e):                                                           # as TSRNEngine._build_layers builds them
        convs = [engine.ConvLayer(e, CP[i] + ".0.weight", CP[i] + ".0.bias", 3, 3, 1, 1, need_dgrad=(i > 0)) for i in range(6)]
        w1 = e.P[FC1 + ".weight"]
        return dict(convs=convs, bns=[engine.BNLayer(e, CP[i] + ".1") for i in range(6)],
                    fc1=engine._FC1AsConv(e, FC1 + ".weight", FC1 + ".bias", w1.shape[0], w1.shape[1] // 2), bnf=engine.BNLayer(e, BNF),
                    fc2=engine.ConvLayer(e, FC2 + ".weight", FC2 + ".bias", wscale=0.1))
    eng = OneLayerEngine(stn_holder(case).to(device), build)
    N = case.N
    d = {k: v.to(device).contiguous() for k, v in case.ins.items()}
    dims, h, w = [], STN_H, STN_W
    for ph, pw in pools:
        dims.append((h, w))
        h, w = h // ph, w // pw
    assert (h, w) == (1, 2) and [N * a * b for a, b in dims] == case.Ms[:6]
    co = [c for _ci, c in STN_CH]
    s = [nan(device, case.Ms[i], co[i]) for i in range(6)]
    ds = [nan(device, case.Ms[i], co[i]) for i in range(6)]
    dz = [nan(device, case.Ms[i], co[i]) for i in range(5)]
    a = [nan(device, N * (dims[i][0] // pools[i][0]) * (dims[i][1] // pools[i][1]), co[i]) for i in range(5)]
    dact = [nan(device, a[i].shape[0], co[i]) for i in range(5)] + [nan(device, N * 2, co[5])]
    f1, ctrl, dfa, df1 = nan(device, N, 512), nan(device, N, 2 * NCTRL), nan(device, N, 512), nan(device, N, 512)

    def fn(eng, L):
        convs, bns, fc1, bnf, fc2 = L["convs"], L["bns"], L["fc1"], L["bnf"], L["fc2"]
        assert convs[0].wt_d is None and (fc1.Cin, fc1.Cout, fc1.KW) == (256, 512, 2) and fc2.wscale == 0.1
        for bn in bns + [bnf]:
            nan_bn(bn, eng._cur_ws)
        nan_scratch(eng, [(c, N, *dims[i]) for i, c in enumerate(convs)] + [(fc1, N, 1, 2), (fc2, N, 1, 1)],
                    [(bn, M) for bn, M in zip(bns + [bnf], case.Ms)])
        cur = d["x"]
        for i, (c, bn, (h, w), (ph, pw)) in enumerate(zip(convs, bns, dims, pools)):      # TSRNEngine._record_stn_fwd
            M = N * h * w
            part, _n = bn.partial(M)
            c.fwd(N, h, w, cur, s[i], bn_partial=part)
            bn.finalize(M, c.b, True)
            if i < 5:
                K.affine_act_pool(s[i], N, h, w, c.Cout, bn.scale, bn.shift, "relu", ph, pw, a[i])
                cur = a[i]
            else:
                cur = s[i]
        part, _n = bnf.partial(N)
        fc1.fwd(N, 1, 2, cur, f1, in_act="relu", bn_partial=part, **bns[5].loader)
        bnf.finalize(N, fc1.b, True)
        fc2.fwd(N, 1, 1, f1, ctrl, in_act="relu", **bnf.loader)
        fc2.wgrad(N, 1, 1, f1, d["dctrl"], loader=dict(in_act="relu", **bnf.loader))    # TSRNEngine._record_stn_bwd, from dctrl
        fc2.dgrad(N, 1, 1, d["dctrl"], dfa)
        bnf.backward(dfa, None, f1, N, "relu", df1)
        fc1.wgrad(N, 1, 2, s[5], df1, loader=dict(in_act="relu", **bns[5].loader))
        fc1.dgrad(N, 1, 2, df1, dact[5])
        for i in range(5, -1, -1):
            c, bn = convs[i], bns[i]
            h, w = dims[i]
            ph, pw = pools[i]
            M = N * h * w
            if i == 5:
                bn.backward(dact[5], None, s[i], M, "relu", ds[i])
            else:
                K.affine_act_pool_bwd(s[i], dact[i], N, h, w, c.Cout, bn.scale, bn.shift, "relu", ph, pw, dz[i])
                bn.backward(dz[i], None, s[i], M, "none", ds[i])
            c.wgrad(N, h, w, a[i - 1] if i > 0 else d["x"], ds[i])
            if i > 0:
                c.dgrad(N, h, w, ds[i], dact[i - 1])

    with launch_log() as names:
        run_engine(eng, fn, device, mode)
    got = {"ctrl": ctrl.cpu()}
    case._grads(eng, got)
    return got, names, {}


# ---- the table the two test files share ----------------------------------------------------------------------------------------------
RUNNERS = {TrunkCase: run_trunk, UpCase: run_up, Block1Case: run_block1, StnCase: run_stn}


def all_cases():
    return trunk_cases() + up_cases() + block1_cases() + [StnCase()]


def run_case(case, device, mode="eager"):
    return RUNNERS[type(case)](case, device, mode)


def compared_keys(case, mode):
    """the running buffers after one forward pass (eager) or after two (recorded); everything else in both"""
    skip = "@2" if mode == "eager" else "@1"
    return [k for k in case.keys if not k.endswith(skip)]


def is_subsequence(part, whole):
    it = iter(whole)
    return all(any(x == y for y in it) for x in part)
