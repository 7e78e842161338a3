"""Every operator of tpgsr_amd/functional.py against stock PyTorch on the CPU in float64, element by element.

Method (the same for every case of the table below): inputs come from a seeded torch.Generator on the CPU; the reference is the stock
PyTorch op in float64 with autograd and a RANDOM upstream gradient; the operator under test runs on the GPU in NHWC with requires_grad on
every differentiable input and parameter, one backward with the same upstream gradient.  Forward values, every input gradient and every
parameter gradient are compared element-wise over the whole tensor: e = max |got - ref| / max |ref|.  Every case runs twice, once with
contiguous activations / upstream gradients and once with non-contiguous ones (permuted or sliced views: the `_c(...)` path of every op).

Where the bounds come from:
  exact  pure data movement: torch.equal against the float32 CPU result.
  arith  arithmetic without a matrix product: e_gpu <= 4 * e_ref32 + 4 * 2^-24, where e_ref32 is the error of stock PyTorch in float32 on
         the CPU against the same float64 reference (4x: the summation order differs; the floor: the fp32 CPU result may be exact).
  conv   operators on the MFMA convolutions, under the policies "x3" and "x2": the limits the raw-kernel tests assert.  x3 (fp32-equivalent):
         5e-6 for values and data gradients (tests/test_kernels_gpu.py::test_conv_fwd_plain), 1e-5 for weight / bias gradients
         (::test_conv_wgrad).  x2 (two bf16 terms per operand, 3 * 2^-18 ~ 1.1e-5 relative per product at worst): 2e-5 for all four
         (tests/test_policy_x2_gpu.py::test_two_term_weight_gradient_error_next_to_fp32_accumulation_noise).  The wrappers add packing,
         tap flipping, dilation and the slab reduce, none of which may add error.

Nothing is masked.  The discontinuous ops get inputs that keep a margin of 1e-3 from their discontinuities (max-pool: top two values of
every window; ReLU / PReLU / signed ReLU: |x|; grid_sample's grid gradient: distance of the un-normalised coordinates from an integer;
the TPS grid's clamp: distance of the source coordinates from 0 and 1); `test_case_table_is_well_posed` asserts those margins, the output
shape formulas and a finite e_ref32 for every case on the CPU.  Max-pool ties are tested separately and exactly.

Observed on an MI355X: worst e_gpu / bound per family (`test_zz_report_worst_ratios` prints the table; for the `arith` rule the bound is
4 * e_ref32 + 4 * 2^-24, so 0.25 means "as accurate as float32 PyTorch on the CPU"; for the `conv` rule it is the policy's limit):
  arith  add 0.09, fork 0.09, batch_norm 0.39, relu 0.00, mish 0.65, tanh 0.58, prelu 0.19, max_pool2d 0.12, upsample_nearest 0.15,
         interpolate_bilinear 0.25, mean_over_height 0.18, grid_sample 0.25, tps_grid+grid_sample 0.10, signed_relu_pool_diff 0.11
  conv   x3: conv2d 0.09, conv2d_strided 0.02, conv_transpose2d 0.10, linear 0.05, PackedLinear 0.04, gru_proj 0.02, bigru 0.05,
             bilstm_eval 0.04
         x2: conv2d 0.40, conv2d_strided 0.40, conv_transpose2d 0.42, linear 0.23, PackedLinear 0.24, gru_proj 0.32, bigru 0.71,
             bilstm_eval 0.49
No family needs more than the 4x margin; every `exact` comparison is bit-exact.
"""
import math
import types
import zlib

import pytest
import torch
import torch.nn.functional as F

DEV = "cuda"
F64 = torch.float64
FLOOR = 4 * 2.0 ** -24
MARGIN = 1e-3
CONV_LIMITS = {"x3": (5e-6, 1e-5), "x2": (2e-5, 2e-5)}          # (values and data gradients, parameter gradients)
POOL_SEEDS = tuple(range(101, 133))                              # max-pool inputs: the first seed whose windows keep the margin


# ---- the case record ---------------------------------------------------------------------------------------------------
class Case:
    """ins: name -> fp32 CPU tensor in the layout the GPU operator takes; acts: the activations among them (fed non-contiguous in the second
    pass); diff: what gets requires_grad; ref(d) / gpu(d): dict of tensors -> tuple of outputs (the first `ngrad` of them differentiable,
    the rest compared only); exact: names compared bit for bit ('*' = all); shape: the expected shape of output 0 (the formula of
    functional.py); margin(d64): asserts the case stays clear of its discontinuities"""

    def __init__(self, family, name, kind, ins, acts, diff, ref, gpu, *, exact=(), shape=None, margin=None, ngrad=1):
        self.family, self.name, self.kind = family, name, kind
        self.ins, self.acts, self.diff, self.ref, self.gpu = ins, tuple(acts), tuple(diff), ref, gpu
        self.exact, self.shape, self.margin, self.ngrad = tuple(exact), shape, margin, ngrad if diff else 0
        self.id = f"{family}-{name}"

    def is_exact(self, key):
        return self.kind == "exact" or "*" in self.exact or key in self.exact


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32("|".join(str(k) for k in key).encode()))


def _away(x, m=2 * MARGIN):
    """push |x| < m out to +-m (zeros go to +m)"""
    s = torch.where(x < 0, -torch.ones_like(x), torch.ones_like(x))
    return torch.where(x.abs() < m, s * m, x)


def _nhwc(x):
    return x.permute(0, 3, 1, 2)


def _nchw(x):
    return x.permute(0, 2, 3, 1)


def _tup(y):
    return y if isinstance(y, tuple) else (y,)


def _upstream(case, outs):
    g = _gen(case.id, "upstream")
    return [torch.randn(o.shape, generator=g) for o in outs[:case.ngrad]]


def run_reference(case, dtype):
    d = {k: v.detach().to(dtype).clone().requires_grad_(k in case.diff) for k, v in case.ins.items()}
    outs = _tup(case.ref(d))
    res = {f"y{i}": o.detach() for i, o in enumerate(outs)}
    if case.ngrad:
        gs = _upstream(case, outs)
        torch.autograd.backward(list(outs[:case.ngrad]), [g.to(dtype) for g in gs])
        for k in case.diff:
            res["d" + k] = d[k].grad if d[k].grad is not None else torch.zeros_like(d[k])
    return res


def _noncontig(t):
    if t.dim() == 4:
        v = t.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
    elif t.dim() >= 1:
        big = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype, device=t.device)
        v = big[..., ::2]
        v.copy_(t)
    else:
        v = t
    return v


def run_gpu(case, nc):
    d = {}
    for k, v in case.ins.items():
        t = v.to(DEV).contiguous()
        if nc and k in case.acts:
            t = _noncontig(t)
        d[k] = t.requires_grad_(k in case.diff)
    outs = _tup(case.gpu(d))
    res = {f"y{i}": o.detach().cpu() for i, o in enumerate(outs)}
    if case.ngrad:
        gs = [g.to(DEV) for g in _upstream(case, [o.detach().cpu() for o in outs])]
        if nc:
            gs = [_noncontig(g) for g in gs]
        torch.autograd.backward(list(outs[:case.ngrad]), gs)
        for k in case.diff:
            assert d[k].grad is not None, f"{case.id}: no gradient for {k}"
            res["d" + k] = d[k].grad.detach().cpu()
    torch.cuda.synchronize()
    return res


def err(got, ref):
    ref = ref.to(F64)
    scale = max(ref.abs().max().item(), 1e-30) if ref.numel() else 1.0
    return ((got.to(F64) - ref).abs().max().item() / scale) if ref.numel() else 0.0


# ---- case table -------------------------------------------------------------------------------------------------------
def _layout_cases():
    from tpgsr_amd import functional as Fh
    out = []
    for i, (N, C, H, W) in enumerate([(2, 1, 3, 5), (2, 3, 4, 7), (1, 4, 1, 9), (2, 37, 5, 1), (1, 64, 6, 11)]):
        x = torch.randn(N, C, H, W, generator=_gen("layout", i))
        out.append(Case("to_nhwc", f"C{C}-{H}x{W}", "exact", {"x": x}, ["x"], ["x"], lambda d: d["x"].permute(0, 2, 3, 1),
                        lambda d: Fh.to_nhwc(d["x"]), shape=(N, H, W, C)))
        xh = x.permute(0, 2, 3, 1).contiguous()
        out.append(Case("to_nchw", f"C{C}-{H}x{W}", "exact", {"x": xh}, ["x"], ["x"], lambda d: d["x"].permute(0, 3, 1, 2),
                        lambda d: Fh.to_nchw(d["x"]), shape=(N, C, H, W)))
    return out


def _ref_conv(d, pad, out_ps=False, wscale=1.0, stride=1):
    x = torch.cat([_nhwc(d["x"]), _nhwc(d["x2"])], 1) if "x2" in d else _nhwc(d["x"])
    y = F.conv2d(x, d["w"] * wscale, d.get("b"), stride=stride, padding=pad)
    return _nchw(F.pixel_shuffle(y, 2) if out_ps else y)


CONV2D = [
    # name, N, H, W, Cin (int, or a pair fed through cat), Cout, (KH, KW), (ph, pw), bias, out_ps, wscale            M = N * OH * OW
    ("3to64-3x3-M63", 1, 7, 9, 3, 64, (3, 3), (1, 1), True, False, 1.0),
    ("3to64-9x9-M1000", 2, 20, 25, 3, 64, (9, 9), (4, 4), True, False, 1.0),
    ("4to12-1x1-M5-nobias", 1, 1, 5, 4, 12, (1, 1), (0, 0), False, False, 1.0),
    ("4to12-3x3-M64", 1, 8, 8, 4, 12, (3, 3), (1, 1), True, False, 1.0),
    ("cat3+32to32-3x3-M65", 5, 1, 13, (3, 32), 32, (3, 3), (1, 1), True, False, 1.0),
    ("64to3-9x9-M64-wscale", 1, 8, 8, 64, 3, (9, 9), (4, 4), True, False, 0.5),
    ("64to256-3x3-M63-pixelshuffle", 1, 7, 9, 64, 256, (3, 3), (1, 1), True, True, 1.0),
    ("64to256-1x1-M1000-nobias", 2, 20, 25, 64, 256, (1, 1), (0, 0), False, False, 1.0),
    ("64to3-2x2p0-M56", 1, 8, 9, 64, 3, (2, 2), (0, 0), True, False, 1.0),
    ("64to256-1x3-M65-wscale", 1, 5, 13, 64, 256, (1, 3), (0, 1), False, False, 1.7),
]


def _conv_cases():
    from tpgsr_amd import functional as Fh
    out = []
    for name, N, H, W, Cin, Cout, k, p, bias, ps, ws in CONV2D:
        g = _gen("conv2d", name)
        cs = Cin if isinstance(Cin, tuple) else (Cin,)
        ins = {"x": torch.randn(N, H, W, cs[0], generator=g)}
        if len(cs) == 2:
            ins["x2"] = torch.randn(N, H, W, cs[1], generator=g)
        ins["w"] = torch.randn(Cout, sum(cs), *k, generator=g) / math.sqrt(sum(cs) * k[0] * k[1])
        if bias:
            ins["b"] = torch.randn(Cout, generator=g)
        OH, OW = H + 2 * p[0] - k[0] + 1, W + 2 * p[1] - k[1] + 1
        acts = [a for a in ("x", "x2") if a in ins]

        def gpu(d, p=p, ps=ps, ws=ws):
            x = Fh.cat([d["x"], d["x2"]]) if "x2" in d else d["x"]
            return Fh.conv2d(x, d["w"], d.get("b"), padding=p, out_ps=ps, wscale=ws)
        out.append(Case("conv2d", name, "conv", ins, acts, list(ins), lambda d, p=p, ps=ps, ws=ws: _ref_conv(d, p, ps, ws), gpu,
                        shape=(N, 2 * OH, 2 * OW, Cout // 4) if ps else (N, OH, OW, Cout)))
    for lead, Cin, Cout, ws in [((7,), 512, 37, 1.0), ((3, 26), 64, 10, 1.0), ((2, 1, 5), 512, 37, 0.25), ((3, 26), 512, 37, 1.0)]:
        g = _gen("linear", lead, Cin)
        ins = {"x": torch.randn(*lead, Cin, generator=g), "w": torch.randn(Cout, Cin, generator=g) / math.sqrt(Cin), "b": torch.randn(Cout, generator=g)}
        out.append(Case("linear", f"{'x'.join(map(str, lead))}-{Cin}to{Cout}", "conv", ins, ["x"], list(ins),
                        lambda d, ws=ws: F.linear(d["x"], d["w"] * ws, d["b"]), lambda d, ws=ws: Fh.linear(d["x"], d["w"], d["b"], wscale=ws),
                        shape=(*lead, Cout)))
    return out


CONVT = [
    # name, N, H, W, Cin, Cout, (KH, KW), stride, padding
    ("s2-k3-p1", 2, 5, 7, 64, 32, (3, 3), (2, 2), (1, 1)),
    ("s2x1-k3x4-p1x2", 2, 5, 7, 32, 16, (3, 4), (2, 1), (1, 2)),
    ("s2x1-k3x5-p1x2", 2, 5, 7, 32, 16, (3, 5), (2, 1), (1, 2)),       # KH - 1 - ph = 1, KW - 1 - pw = 2: swapping them shows
    ("s1x2-k4x3-p2x0", 1, 6, 5, 16, 8, (4, 3), (1, 2), (2, 0)),
    ("s1-k3-p1", 2, 5, 7, 32, 32, (3, 3), (1, 1), (1, 1)),
    ("infogen1-37to512", 2, 1, 26, 37, 512, (3, 3), (2, 2), (1, 1)),
    ("infogen2-512to128", 2, 1, 51, 512, 128, (3, 3), (2, 2), (1, 1)),
    ("infogen3-128to64", 2, 1, 101, 128, 64, (3, 3), (2, 2), (1, 1)),
    ("infogen4-64to32-s2x1-p1x0", 2, 1, 201, 64, 32, (3, 3), (2, 1), (1, 0)),
    ("infogen-tl-p0", 2, 1, 5, 64, 128, (3, 3), (2, 2), (0, 0)),
]
STRIDED = [
    # name, N, H, W, stride, zero-fill branch of _Subsample.backward ((H - 1) % sh or (W - 1) % sw)
    ("s2x1-7x9-nofill", 2, 7, 9, (2, 1), False),
    ("s2x1-8x9-fillrows", 2, 8, 9, (2, 1), True),
    ("s2x2-7x9-nofill", 2, 7, 9, (2, 2), False),
    ("s2x2-8x10-fill", 2, 8, 10, (2, 2), True),
    ("s2x2-7x10-fillcols", 1, 7, 10, (2, 2), True),
    ("s3x2-6x6-fill", 1, 6, 6, (3, 2), True),
]


def _convt_strided_cases():
    from tpgsr_amd import functional as Fh
    out = []
    for name, N, H, W, Cin, Cout, k, s, p in CONVT:
        g = _gen("convT", name)
        ins = {"x": torch.randn(N, H, W, Cin, generator=g), "w": torch.randn(Cin, Cout, *k, generator=g) / math.sqrt(Cin * k[0] * k[1])}
        # the equivalent stride-1 conv of functional.conv_transpose2d: over the dilated map, padding KH - 1 - ph
        HD, WD = (H - 1) * s[0] + 1, (W - 1) * s[1] + 1
        shape = (N, HD + 2 * (k[0] - 1 - p[0]) - k[0] + 1, WD + 2 * (k[1] - 1 - p[1]) - k[1] + 1, Cout)
        out.append(Case("conv_transpose2d", name, "conv", ins, ["x"], ["x", "w"],
                        lambda d, s=s, p=p: _nchw(F.conv_transpose2d(_nhwc(d["x"]), d["w"], None, stride=s, padding=p)),
                        lambda d, s=s, p=p: Fh.conv_transpose2d(d["x"], d["w"], stride=s, padding=p), shape=shape))
    for name, N, H, W, s, fill in STRIDED:
        g = _gen("strided", name)
        assert fill == bool((H - 1) % s[0] or (W - 1) % s[1])
        ins = {"x": torch.randn(N, H, W, 8, generator=g), "w": torch.randn(16, 8, 3, 3, generator=g) / math.sqrt(72), "b": torch.randn(16, generator=g)}
        shape = (N, (H + s[0] - 1) // s[0], (W + s[1] - 1) // s[1])
        out.append(Case("conv2d_strided", name, "conv", ins, ["x"], list(ins), lambda d, s=s: _ref_conv(d, (1, 1), stride=s),
                        lambda d, s=s: Fh.conv2d_strided(d["x"], d["w"], d["b"], stride=s, padding=1), shape=(*shape, 16)))
        xs = {"x": torch.randn(N, H, W, 5, generator=g)}
        out.append(Case("subsample", name, "exact", xs, ["x"], ["x"], lambda d, s=s: d["x"][:, ::s[0], ::s[1]],
                        lambda d, s=s: Fh.subsample(d["x"], s[0], s[1]), shape=(*shape, 5)))

        def dil(d, s=s):
            x = d["x"]
            z = torch.zeros(x.shape[0], (x.shape[1] - 1) * s[0] + 1, (x.shape[2] - 1) * s[1] + 1, x.shape[3], dtype=x.dtype)
            ih, iw = torch.arange(x.shape[1]) * s[0], torch.arange(x.shape[2]) * s[1]
            return z.index_put((torch.arange(x.shape[0])[:, None, None], ih[None, :, None], iw[None, None, :]), x)
        out.append(Case("dilate", name, "exact", xs, ["x"], ["x"], dil, lambda d, s=s: Fh._Dilate.apply(d["x"], s[0], s[1]),
                        shape=(N, (H - 1) * s[0] + 1, (W - 1) * s[1] + 1, 5)))
    return out


BN = [
    # name, (N, H, W), C, act                        M = N * H * W: nblk = max(1, min(1024, M // 64)), ragged last block
    ("M8-C4", (2, 2, 2), 4, None),
    ("M63-C8-relu", (1, 7, 9), 8, "relu"),
    ("M64-C64-mish", (1, 8, 8), 64, "mish"),
    ("M90-C128", (2, 5, 9), 128, None),
    ("M90-C64-relu", (2, 5, 9), 64, "relu"),
    ("M4113-C8-relu", (3, 3, 457), 8, "relu"),
    ("M4113-C64-mish", (3, 3, 457), 64, "mish"),
    ("M4113-C128", (3, 3, 457), 128, None),
]


def _bn_ref(d, act, training, momentum=0.1, eps=1e-5):
    rm, rv = d["rm"].detach().clone(), d["rv"].detach().clone()
    y = F.batch_norm(_nhwc(d["x"]), rm, rv, d["gamma"], d["beta"], training, momentum, eps)
    y = F.relu(y) if act == "relu" else (F.mish(y) if act == "mish" else y)
    return _nchw(y), rm, rv


def _bn_holder(d, momentum=0.1, eps=1e-5):
    return types.SimpleNamespace(weight=d["gamma"], bias=d["beta"], running_mean=d["rm"].detach().clone(), running_var=d["rv"].detach().clone(),
                                 momentum=momentum, eps=eps, num_batches_tracked=torch.tensor(0, dtype=torch.long))


def _bn_cases():
    from tpgsr_amd import functional as Fh
    out = []
    for name, nhw, C, act in BN:
        g = _gen("bn", name)
        ins = {"x": torch.randn(*nhw, C, generator=g) * 1.5 + 0.3, "gamma": torch.rand(C, generator=g) + 0.5, "beta": torch.randn(C, generator=g) * 0.3,
               "rm": torch.randn(C, generator=g) * 0.2, "rv": torch.rand(C, generator=g) + 0.5}
        pre = lambda x, i=ins: _bn_ref({**{k: v.to(F64) for k, v in i.items()}, "x": x.to(F64)}, None, True)[0]
        if act == "relu":       # move the inputs whose normalised value sits within the margin of the ReLU's kink (the statistics move with them)
            for _ in range(50):
                z = pre(ins["x"])
                bad = z.abs() < 2 * MARGIN
                if not bad.any():
                    break
                ins["x"] = torch.where(bad, ins["x"] + 0.02 * torch.where(z < 0, -1.0, 1.0).float(), ins["x"])

        def gpu(d, act=act):
            bn = _bn_holder(d)
            y = Fh.batch_norm(d["x"], bn, True, act)
            assert int(bn.num_batches_tracked) == 1
            return y, bn.running_mean, bn.running_var
        margin = (lambda d64, pre=pre: _assert_margin(pre(d64["x"]).abs().min().item(), "BatchNorm output to the ReLU kink")) if act == "relu" else None
        out.append(Case("batch_norm", name, "arith", ins, ["x"], ["x", "gamma", "beta"], lambda d, act=act: _bn_ref(d, act, True), gpu,
                        shape=(*nhw, C), margin=margin))
    g = _gen("bn", "eval")
    ins = {"x": torch.randn(2, 5, 9, 8, generator=g), "gamma": torch.rand(8, generator=g) + 0.5, "beta": torch.randn(8, generator=g) * 0.3,
           "rm": torch.randn(8, generator=g) * 0.2, "rv": torch.rand(8, generator=g) + 0.5}

    def gpu_eval(d):
        bn = _bn_holder(d)
        y = Fh.batch_norm(d["x"], bn, False, "mish")
        assert int(bn.num_batches_tracked) == 0
        return y, bn.running_mean, bn.running_var
    out.append(Case("batch_norm", "eval-M90-C8-mish", "arith", ins, ["x"], [], lambda d: _bn_ref(d, "mish", False), gpu_eval, shape=(2, 5, 9, 8)))
    return out


def _assert_margin(value, what, m=MARGIN):
    assert value >= m, f"{what}: margin {value:.3e} < {m:.0e}"


def _elementwise_cases():
    from tpgsr_amd import functional as Fh
    out = []
    refs = {"relu": F.relu, "mish": F.mish, "tanh": torch.tanh}
    for act in ("relu", "mish", "tanh"):
        for name, shape, scale in [("n4", (1, 1, 1, 4), 1.0), ("n1260", (2, 5, 7, 18), 2.0), ("n65536+4", (1, 1, 16385, 4), 1.0), ("big-magnitude", (2, 3, 8, 8), 12.0)]:
            g = _gen("act", act, name)
            x = torch.randn(*shape, generator=g) * scale
            if name == "big-magnitude":
                x = (torch.rand(*shape, generator=g) * 60.0 - 30.0)          # |x| up to 30: softplus overflow region of mish, saturated tanh
                x.view(-1)[:6] = torch.tensor([-30.0, 30.0, 20.0, 20.5, -20.0, 19.999])
            if act == "relu":
                x = _away(x)
            margin = (lambda d64: _assert_margin(d64["x"].abs().min().item(), "|x| of a ReLU input")) if act == "relu" else None
            out.append(Case(act, name, "arith", {"x": x}, ["x"], ["x"], lambda d, f=refs[act]: f(d["x"]), lambda d, f=getattr(Fh, act): f(d["x"]),
                            shape=shape, margin=margin))
    for name, n, alpha in [("n4-neg", 4, -0.3), ("n1024-zero", 1024, 0.0), ("n3076-gt1", 256 * 4 * 3 + 4, 1.7), ("n3076-quarter", 256 * 4 * 3 + 4, 0.25),
                           ("n262156-all-256-blocks", 4 * (256 * 256 + 3), 0.25)]:      # every one of the 256 partial sums of d alpha carries data
        g = _gen("prelu", name)
        ins = {"x": _away(torch.randn(1, n // 4, 1, 4, generator=g)), "alpha": torch.tensor([alpha])}
        out.append(Case("prelu", name, "arith", ins, ["x"], ["x", "alpha"], lambda d: F.prelu(d["x"], d["alpha"]), lambda d: Fh.prelu(d["x"], d["alpha"]),
                        shape=(1, n // 4, 1, 4), margin=lambda d64: _assert_margin(d64["x"].abs().min().item(), "|x| of a PReLU input")))
    for name, shape in [("4d", (2, 3, 5, 8)), ("3d-odd", (3, 7, 5)), ("n1", (1, 1, 1, 1))]:
        g = _gen("add", name)
        ins = {"a": torch.randn(*shape, generator=g), "b": torch.randn(*shape, generator=g)}
        out.append(Case("add", name, "arith", ins, ["a", "b"], ["a", "b"], lambda d: d["a"] + d["b"], lambda d: Fh.add(d["a"], d["b"]), shape=shape))
        x = {"x": torch.randn(*shape, generator=g)}
        out.append(Case("fork", name + "-both", "arith", x, ["x"], ["x"], lambda d: (d["x"] * 1, d["x"] * 1), lambda d: Fh.fork(d["x"]), shape=shape,
                        exact=("y0", "y1"), ngrad=2))
        out.append(Case("fork", name + "-one-unused", "exact", x, ["x"], ["x"], lambda d: d["x"] * 1, lambda d: Fh.fork(d["x"])[1], shape=shape))
    for name, lead, cs in [("64+32", (2, 3, 5), (64, 32)), ("3+32", (1, 4, 7), (3, 32)), ("1+1", (2, 2, 3), (1, 1)), ("37+5+22", (2, 1, 9), (37, 5, 22)),
                           ("3d-64+32", (3, 26), (64, 32)), ("3d-37+5+22", (2, 7), (37, 5, 22))]:
        g = _gen("cat", name)
        ins = {f"x{i}": torch.randn(*lead, c, generator=g) for i, c in enumerate(cs)}
        out.append(Case("cat", name, "exact", ins, list(ins), list(ins), lambda d: torch.cat([d[k] for k in sorted(d)], -1),
                        lambda d: Fh.cat([d[k] for k in sorted(d)]), shape=(*lead, sum(cs))))
    return out


POOL = [
    # name, (N, H, W, C), kernel, stride, padding
    ("2x2s2-even-vec", (2, 6, 10, 8), (2, 2), (2, 2), (0, 0)),        # the 2x2 fast backward path
    ("2x2s2-odd-vec", (2, 5, 9, 8), (2, 2), (2, 2), (0, 0)),          # the gather form; last row / column in no window
    ("2x2s2-even-C3", (1, 6, 10, 3), (2, 2), (2, 2), (0, 0)),         # scalar kernels
    ("2x2s2x1p0x1-evenH", (2, 4, 9, 8), (2, 2), (2, 1), (0, 1)),      # the stride-(2, 1) fast path, windows over the padding
    ("2x2s2x1p0x1-oddH", (2, 5, 9, 8), (2, 2), (2, 1), (0, 1)),
    ("3x3s2p1-7x9", (2, 7, 9, 4), (3, 3), (2, 2), (1, 1)),
    ("3x3s2p1-8x10-C5", (1, 8, 10, 5), (3, 3), (2, 2), (1, 1)),
    ("3x3s1p0-overlap", (1, 6, 7, 4), (3, 3), (1, 1), (0, 0)),
    ("3x2s1x2p1x0", (2, 5, 8, 4), (3, 2), (1, 2), (1, 0)),
]


def _top2_gap(x_nchw, k, s, p):
    xp = F.pad(x_nchw, (p[1], p[1], p[0], p[0]), value=float("-inf"))
    u = F.unfold(xp, k, stride=s).view(x_nchw.shape[0], x_nchw.shape[1], k[0] * k[1], -1)
    t = u.topk(2, dim=2).values
    return (t[:, :, 0] - t[:, :, 1]).min().item()


def _pool_out(H, W, k, s, p):
    return (H + 2 * p[0] - k[0]) // s[0] + 1, (W + 2 * p[1] - k[1]) // s[1] + 1


def _pool_cases():
    from tpgsr_amd import functional as Fh
    out = []
    for name, (N, H, W, C), k, s, p in POOL:
        x = None
        for seed in POOL_SEEDS:
            x = torch.randn(N, H, W, C, generator=torch.Generator().manual_seed(seed)) * 3.0
            if _top2_gap(_nhwc(x).double(), k, s, p) >= 2 * MARGIN:
                break
        OH, OW = _pool_out(H, W, k, s, p)
        out.append(Case("max_pool2d", name, "arith", {"x": x}, ["x"], ["x"], lambda d, k=k, s=s, p=p: _nchw(F.max_pool2d(_nhwc(d["x"]), k, s, p)),
                        lambda d, k=k, s=s, p=p: Fh.max_pool2d(d["x"], k, s, p), exact=("y0",), shape=(N, OH, OW, C),
                        margin=lambda d64, k=k, s=s, p=p: _assert_margin(_top2_gap(_nhwc(d64["x"]), k, s, p), "top two values of a max-pool window")))
    for name, (N, H, W, C), k, s in [("k2s1", (2, 5, 9, 1), 2, 1), ("k2s2", (2, 6, 9, 4), 2, 2), ("k2s1-C4", (1, 4, 26, 4), 2, 1)]:
        x = _away(torch.randn(N, H, W, C, generator=_gen("srpd", name)))
        out.append(Case("signed_relu_pool_diff", name, "arith", {"x": x}, ["x"], [],
                        lambda d, k=k, s=s: _nchw(F.max_pool2d(F.relu(_nhwc(d["x"])), k, s) - F.max_pool2d(F.relu(-_nhwc(d["x"])), k, s)),
                        lambda d, k=k, s=s: Fh.signed_relu_pool_diff(d["x"], k, s), shape=(N, (H - k) // s + 1, (W - k) // s + 1, C),
                        margin=lambda d64: _assert_margin(d64["x"].abs().min().item(), "|x| of a signed-ReLU input")))
    for name, (N, H, W) in [("8x25", (2, 8, 25)), ("1x1", (1, 1, 1))]:
        g = _gen("offgrid", name)
        ins = {"grid": torch.rand(N, H, W, 2, generator=g) * 2 - 1, "dy": torch.randn(N, H, W, 1, generator=g) * 0.1}
        out.append(Case("offset_grid_y", name, "exact", ins, ["grid", "dy"], [], lambda d: torch.cat([d["grid"][..., :1], d["grid"][..., 1:] + d["dy"]], -1),
                        lambda d: Fh.offset_grid_y(d["grid"], d["dy"]), shape=(N, H, W, 2)))
    return out


def _resample_cases():
    from tpgsr_amd import functional as Fh
    out = []
    for s in (1, 2, 3):
        for (N, H, W, C) in [(2, 3, 5, 4), (1, 1, 7, 3)]:
            x = torch.randn(N, H, W, C, generator=_gen("nearest", s, C))
            out.append(Case("upsample_nearest", f"x{s}-{H}x{W}-C{C}", "arith", {"x": x}, ["x"], ["x"],
                            lambda d, s=s: _nchw(F.interpolate(_nhwc(d["x"]), scale_factor=s, mode="nearest")),
                            lambda d, s=s: Fh.upsample_nearest(d["x"], s), exact=("y0",), shape=(N, H * s, W * s, C)))
    for (H, W), (OH, OW) in [((1, 26), (16, 64)), ((16, 64), (32, 64)), ((5, 7), (5, 7)), ((8, 8), (1, 1)), ((1, 1), (4, 4)), ((3, 50), (2, 13)),
                             ((16, 64), (8, 32)), ((2, 2), (7, 5))]:
        for C in (4, 5):
            x = torch.randn(2, H, W, C, generator=_gen("bilinear", H, W, OH, OW, C))
            out.append(Case("interpolate_bilinear", f"{H}x{W}-to-{OH}x{OW}-C{C}", "arith", {"x": x}, ["x"], ["x"],
                            lambda d, o=(OH, OW): _nchw(F.interpolate(_nhwc(d["x"]), size=o, mode="bilinear", align_corners=True)),
                            lambda d, o=(OH, OW): Fh.interpolate_bilinear(d["x"], o), shape=(2, OH, OW, C)))
    for H in (1, 2, 3):
        for C in (512, 5):
            x = torch.randn(2, H, 26, C, generator=_gen("hmean", H, C))
            out.append(Case("mean_over_height", f"H{H}-C{C}", "arith", {"x": x}, ["x"], ["x"], lambda d: d["x"].mean(1),
                            lambda d: Fh.mean_over_height(d["x"]), shape=(2, 26, C)))
    return out


_GRU_NAMES = ("w_ih", "w_hh", "b_ih", "b_hh", "w_ih_r", "w_hh_r", "b_ih_r", "b_hh_r")
_RNN_KEYS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0", "weight_ih_l0_reverse", "weight_hh_l0_reverse", "bias_ih_l0_reverse",
             "bias_hh_l0_reverse")


def _rnn_ref(cls, seq, d, hidden):
    from torch.func import functional_call
    net = cls(seq.shape[-1], hidden, bidirectional=True, batch_first=True).to(seq.dtype)
    return functional_call(net, {k: d[n] for k, n in zip(_RNN_KEYS, _GRU_NAMES)}, (seq,))[0]


def _gru_ref(d, axis):
    x = d["x"]
    N, H, W, Cin = x.shape
    if axis == 0:
        return _rnn_ref(torch.nn.GRU, x.reshape(N * H, W, Cin), d, 32).reshape(N, H, W, 64)
    return _rnn_ref(torch.nn.GRU, x.permute(0, 2, 1, 3).reshape(N * W, H, Cin), d, 32).reshape(N, W, H, 64).permute(0, 2, 1, 3)


def _rnn_params(g, Cin, Hh, gates):
    b = 1.0 / math.sqrt(Hh)
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) * b
    p = {}
    for suf in ("", "_r"):
        p["w_ih" + suf], p["w_hh" + suf], p["b_ih" + suf], p["b_hh" + suf] = u(gates * Hh, Cin), u(gates * Hh, Hh), u(gates * Hh), u(gates * Hh)
    return p


def _gru_holder(d):
    return types.SimpleNamespace(**{k: d[n] for k, n in zip(_RNN_KEYS, _GRU_NAMES)})


def _recurrent_cases():
    from tpgsr_amd import functional as Fh
    out = []
    for axis in (0, 1):
        for (N, H, W), Cin in [((1, 1, 1), 64), ((2, 3, 5), 96), ((3, 16, 64), 64), ((2, 3, 5), 64)]:
            g = _gen("bigru", axis, N, H, W, Cin)
            ins = {"x": torch.randn(N, H, W, Cin, generator=g), **_rnn_params(g, Cin, 32, 3)}
            out.append(Case("bigru", f"axis{axis}-{N}x{H}x{W}-C{Cin}", "conv", ins, ["x"], list(ins), lambda d, a=axis: _gru_ref(d, a),
                            lambda d, a=axis: Fh.bigru(d["x"], _gru_holder(d), a), shape=(N, H, W, 64)))
    for (N, H, W), Cin in [((2, 3, 5), 96), ((1, 7, 10), 64)]:       # both column halves of gi, each written by its own launch
        g = _gen("gruproj", N, H, W, Cin)
        p = _rnn_params(g, Cin, 32, 3)
        ins = {"x": torch.randn(N, H, W, Cin, generator=g), "w0": p["w_ih"], "w1": p["w_ih_r"], "b0": p["b_ih"], "b1": p["b_ih_r"]}
        out.append(Case("gru_proj", f"{N}x{H}x{W}-C{Cin}", "conv", ins, ["x"], list(ins),
                        lambda d: torch.cat([F.linear(d["x"], d["w0"], d["b0"]), F.linear(d["x"], d["w1"], d["b1"])], -1),
                        lambda d: Fh._GruProj.apply(d["x"], d["w0"], d["w1"], d["b0"], d["b1"]), shape=(N, H, W, 192)))
    for rows, Cin, Cout in [(1, 512, 37), (26, 64, 10), (130, 512, 37), (130, 64, 256)]:
        g = _gen("packed", rows, Cin)
        ins = {"x": torch.randn(rows, Cin, generator=g), "w": torch.randn(Cout, Cin, generator=g) / math.sqrt(Cin), "b": torch.randn(Cout, generator=g)}
        out.append(Case("PackedLinear", f"rows{rows}-{Cin}to{Cout}", "conv", ins, ["x"], [], lambda d: F.linear(d["x"], d["w"], d["b"]),
                        lambda d: Fh.PackedLinear(d["w"], d["b"])(d["x"]), shape=(rows, Cout)))

        def gpu_out(d, rows=rows, Cout=Cout):
            big = torch.full((rows + 7, Cout), 123.0, device=d["x"].device)
            y = Fh.PackedLinear(d["w"], d["b"])(d["x"], out=big[3:3 + rows])
            assert y.data_ptr() == big[3:].data_ptr()
            return big

        def ref_out(d, rows=rows, Cout=Cout):
            big = torch.full((rows + 7, Cout), 123.0, dtype=d["x"].dtype)
            big[3:3 + rows] = F.linear(d["x"], d["w"], d["b"])
            return big
        out.append(Case("PackedLinear", f"rows{rows}-{Cin}to{Cout}-out-rowblock", "conv", ins, ["x"], [], ref_out, gpu_out, shape=(rows + 7, Cout)))
    for Hh in (256, 32):
        for T in (1, 26):
            g = _gen("bilstm", Hh, T)
            ins = {"x": torch.randn(3, T, 64, generator=g), **_rnn_params(g, 64, Hh, 4)}
            out.append(Case("bilstm_eval", f"Hh{Hh}-T{T}", "conv", ins, ["x"], [], lambda d, Hh=Hh: _rnn_ref(torch.nn.LSTM, d["x"], d, Hh),
                            lambda d: Fh.bilstm_eval(d["x"], *[d[n] for n in _GRU_NAMES]), shape=(3, T, 2 * Hh)))
    return out


def _unnorm(g, size, align):
    return (g + 1) * 0.5 * (size - 1) if align else ((g + 1) * size - 1) * 0.5


def _grid_int_gap(grid64, H, W, align):
    ix, iy = _unnorm(grid64[..., 0], W, align), _unnorm(grid64[..., 1], H, align)
    return min((ix - ix.round()).abs().min().item(), (iy - iy.round()).abs().min().item())


def _tps_consts(th, tw):
    from tpgsr_amd.model.tps_spatial_transformer import TPSSpatialTransformer
    t = TPSSpatialTransformer(output_image_size=(th, tw), num_control_points=20, margins=(0.05, 0.05))
    return t.inverse_kernel.clone(), t.target_coordinate_repr.clone(), t.target_control_points.clone()


def _tps_src(d):
    ctrl = d["ctrl"]
    Y = torch.cat([ctrl, torch.zeros(ctrl.shape[0], 3, 2, dtype=ctrl.dtype)], 1)
    return torch.matmul(d["repr"], torch.matmul(d["invk"], Y))


def _tps_ref(d, th, tw, align):
    grid = 2.0 * _tps_src(d).clamp(0, 1) - 1.0
    y = _nchw(F.grid_sample(_nhwc(d["x"]), grid.view(-1, th, tw, 2), mode="bilinear", padding_mode="zeros", align_corners=align))
    return y, grid


TPS_SEEDS = tuple(range(201, 713))


def _tps_margins(d64, H, W, align):
    """(distance of the source coordinates from the clamp's kinks at 0 and 1, distance of the un-normalised coordinates of the UNCLAMPED
    points from an integer: a clamped coordinate sits on a pixel centre or edge exactly, and the clamp hands its gradient a zero)"""
    src = _tps_src(d64)
    clamp_gap = min(src.abs().min().item(), (src - 1).abs().min().item())
    inside = (src > 0) & (src < 1)
    u = torch.stack([_unnorm(2 * src[..., 0] - 1, W, align), _unnorm(2 * src[..., 1] - 1, H, align)], -1)
    gap = (u - u.round()).abs()
    return clamp_gap, (gap[inside].min().item() if inside.any() else 1.0)


def _stn_cases():
    from tpgsr_amd import functional as Fh
    out = []
    for C, align, (H, W), (th, tw), diff in [(3, False, (6, 11), (4, 9), ("x", "ctrl")), (4, True, (5, 8), (4, 9), ("x", "ctrl")), (1, False, (7, 7), (3, 8), ("x", "ctrl")),
                                            (4, False, (6, 11), (4, 9), ("ctrl",)), (3, True, (6, 11), (4, 9), ("x",))]:
        invk, rep, tcp = _tps_consts(th, tw)
        ins = None
        for seed in TPS_SEEDS:       # perturbed control points: the first seed that keeps both margins (the clamp at 0 / 1, the sampler's floor)
            g = torch.Generator().manual_seed(seed)
            ins = {"x": torch.randn(2, H, W, C, generator=g), "ctrl": tcp[None] + torch.randn(2, 20, 2, generator=g) * 0.04, "invk": invk, "repr": rep}
            if min(_tps_margins({k: v.double() for k, v in ins.items()}, H, W, align)) >= 2 * MARGIN:
                break

        def margin(d64, H=H, W=W, align=align):
            clamp_gap, int_gap = _tps_margins(d64, H, W, align)
            _assert_margin(clamp_gap, "TPS source coordinates to the clamp at 0 / 1")
            _assert_margin(int_gap, "un-normalised sample coordinates to an integer")
            src = _tps_src(d64)
            assert ((src < 0) | (src > 1)).any() and ((src > 0) & (src < 1)).any()          # both sides of the clamp are exercised

        def gpu(d, th=th, tw=tw, align=align):
            grid, _src = Fh.tps_grid(d["ctrl"], d["invk"], d["repr"], th * tw)
            return Fh.grid_sample(d["x"], grid, (th, tw), align), grid.detach()
        out.append(Case("tps_grid+grid_sample", f"C{C}-align{int(align)}-{H}x{W}-to-{th}x{tw}-d{'+'.join(diff)}", "arith", ins, ["x", "ctrl"], list(diff),
                        lambda d, th=th, tw=tw, align=align: _tps_ref(d, th, tw, align), gpu, shape=(2, th, tw, C), margin=margin))
    for C, align, (H, W), (OH, OW), diff in [(3, False, (6, 11), (5, 13), ("x", "grid")), (4, True, (6, 11), (5, 13), ("x", "grid")), (1, True, (4, 4), (9, 3), ("x", "grid")),
                                            (4, False, (5, 8), (3, 7), ("grid",)), (1, False, (5, 8), (3, 7), ("x",))]:
        g = _gen("gridsample", C, align, H, W)
        # un-normalised coordinates from two pixels outside the map on either side, pushed away from the integers, then normalised
        ix = torch.rand(2, OH, OW, generator=g, dtype=F64) * (W + 3) - 2
        iy = torch.rand(2, OH, OW, generator=g, dtype=F64) * (H + 3) - 2
        fr = lambda v: v.floor() + (v - v.floor()).clamp(0.01, 0.99)
        ix, iy = fr(ix), fr(iy)
        nx = (2 * ix / (W - 1) - 1) if align else ((2 * ix + 1) / W - 1)
        ny = (2 * iy / (H - 1) - 1) if align else ((2 * iy + 1) / H - 1)
        ins = {"x": torch.randn(2, H, W, C, generator=g), "grid": torch.stack([nx, ny], -1).float()}
        out.append(Case("grid_sample", f"C{C}-align{int(align)}-{H}x{W}-to-{OH}x{OW}-d{'+'.join(diff)}", "arith", ins, ["x", "grid"], list(diff),
                        lambda d, align=align: _nchw(F.grid_sample(_nhwc(d["x"]), d["grid"], mode="bilinear", padding_mode="zeros", align_corners=align)),
                        lambda d, o=(OH, OW), align=align: Fh.grid_sample(d["x"], d["grid"], o, align), shape=(2, OH, OW, C),
                        margin=lambda d64, H=H, W=W, align=align: _assert_margin(_grid_int_gap(d64["grid"], H, W, align), "un-normalised sample coordinates to an integer")))
    for C, align in [(3, False), (4, True), (1, False), (4, False)]:
        # the forward (and the image gradient) is continuous in the grid: exact pixel centres, exact -1 / +1, points outside [-1, 1]
        H, W, OH, OW = 5, 9, 4, 12
        g = _gen("gridsample-special", C, align)
        px = torch.randint(0, W, (2, OH, OW), generator=g).double()
        py = torch.randint(0, H, (2, OH, OW), generator=g).double()
        nx = (2 * px / (W - 1) - 1) if align else ((2 * px + 1) / W - 1)
        ny = (2 * py / (H - 1) - 1) if align else ((2 * py + 1) / H - 1)
        grid = torch.stack([nx, ny], -1).float()
        grid[:, 0, :6] = torch.tensor([[-1.0, -1.0], [1.0, 1.0], [-1.0, 1.0], [1.0, -1.0], [0.0, 0.0], [1.0, 0.3]])
        grid[:, 1, :6] = torch.tensor([[-1.5, 0.2], [1.25, -0.4], [0.1, 1.75], [0.3, -2.0], [-3.0, -3.0], [2.5, 2.5]])
        ins = {"x": torch.randn(2, H, W, C, generator=g), "grid": grid}
        out.append(Case("grid_sample", f"special-points-C{C}-align{int(align)}", "arith", ins, ["x", "grid"], ["x"],
                        lambda d, align=align: _nchw(F.grid_sample(_nhwc(d["x"]), d["grid"], mode="bilinear", padding_mode="zeros", align_corners=align)),
                        lambda d, o=(OH, OW), align=align: Fh.grid_sample(d["x"], d["grid"], o, align), shape=(2, OH, OW, C)))
    return out


_CASES = None


def all_cases():
    global _CASES
    if _CASES is None:
        _CASES = (_layout_cases() + _conv_cases() + _convt_strided_cases() + _bn_cases() + _elementwise_cases() + _pool_cases() + _resample_cases() +
                  _recurrent_cases() + _stn_cases())
        ids = [c.id for c in _CASES]
        assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return _CASES


def _params():
    ps = []
    for c in all_cases():
        for pol in (("x3", "x2") if c.kind == "conv" else (None,)):
            ps.append(pytest.param(c, pol, id=c.id + (f"-{pol}" if pol else ""), marks=pytest.mark.gpu))
    return ps


# ---- CPU: the table is well posed ------------------------------------------------------------------------------------------
def test_case_table_is_well_posed():
    """Every case of the table, on the CPU: (a) it keeps its margin from the discontinuities of its op, (b) the float32 reference's error
    against float64 is finite (and passes the rule it defines, trivially), (c) output 0 has the shape functional.py's formulas give
    (_MaxPool, _Dilate, _Subsample, the transposed convolution's padding KH - 1 - ph) -- and the float64 reference gives every gradient."""
    cases = all_cases()
    fams = {c.family for c in cases}
    assert {"to_nhwc", "to_nchw", "conv2d", "linear", "conv_transpose2d", "conv2d_strided", "subsample", "dilate", "batch_norm", "relu", "mish", "tanh",
            "prelu", "add", "fork", "cat", "max_pool2d", "upsample_nearest", "interpolate_bilinear", "mean_over_height", "bigru", "gru_proj",
            "tps_grid+grid_sample", "grid_sample", "PackedLinear", "bilstm_eval", "signed_relu_pool_diff", "offset_grid_y"} <= fams
    for c in cases:
        assert all(v.dtype == torch.float32 and v.numel() * 4 < 8 << 20 for v in c.ins.values()), c.id
        if c.margin is not None:
            c.margin({k: v.double() for k, v in c.ins.items()})
        r64, r32 = run_reference(c, F64), run_reference(c, torch.float32)
        assert tuple(r64["y0"].shape) == tuple(c.shape), (c.id, tuple(r64["y0"].shape), c.shape)
        assert set(r64) == set(r32) and all(("d" + k) in r64 for k in c.diff), c.id
        for key in r64:
            assert r64[key].dtype == F64 and r32[key].dtype == torch.float32 and r64[key].shape == r32[key].shape, (c.id, key)
            e32 = err(r32[key], r64[key])
            assert math.isfinite(e32) and torch.isfinite(r64[key]).all(), (c.id, key, e32)
            assert e32 <= 4 * e32 + FLOOR
            if c.is_exact(key):
                assert e32 <= 2.0 ** -23, (c.id, key, e32)       # data movement: float32 reproduces float64 up to the rounding of the values


def test_cpu_and_dtype_guards(monkeypatch):
    """a CPU tensor raises RuntimeError (no stock-PyTorch fallback); an fp16 / fp64 tensor raises TypeError -- checked on the CPU through the
    plan dry-run switch, which stands in for 'is a CUDA tensor' in functional._chk; both refusals come before any launch"""
    from tpgsr_amd import functional as Fh, kernels as K
    x = torch.randn(1, 2, 3, 4)
    w = torch.randn(4, 4, 1, 1)
    bn = types.SimpleNamespace(weight=torch.ones(4), bias=torch.zeros(4), running_mean=torch.zeros(4), running_var=torch.ones(4), momentum=0.1, eps=1e-5,
                               num_batches_tracked=torch.tensor(0))
    calls = [lambda t: Fh.to_nhwc(t), lambda t: Fh.to_nchw(t), lambda t: Fh.conv2d(t, w.to(t.dtype)), lambda t: Fh.relu(t), lambda t: Fh.prelu(t, torch.ones(1, dtype=t.dtype)),
             lambda t: Fh.add(t, t), lambda t: Fh.fork(t), lambda t: Fh.cat([t, t]), lambda t: Fh.max_pool2d(t, 2), lambda t: Fh.upsample_nearest(t, 2),
             lambda t: Fh.interpolate_bilinear(t, (4, 4)), lambda t: Fh.mean_over_height(t), lambda t: Fh.subsample(t, 2, 2), lambda t: Fh.batch_norm(t, bn, False),
             lambda t: Fh.grid_sample(t, torch.zeros(1, 2, 2, 2, dtype=t.dtype), (2, 2)), lambda t: Fh.signed_relu_pool_diff(t, 2, 1),
             lambda t: Fh.offset_grid_y(t[..., :2], t[..., :1]), lambda t: Fh.PackedLinear(w.to(t.dtype).view(4, 4))(t)]
    monkeypatch.setattr(K, "DRYRUN", False)
    for f in calls:
        with pytest.raises(RuntimeError, match="GPU only"):
            f(x)
    monkeypatch.setattr(K, "DRYRUN", True)
    for f in calls:
        for dt in (torch.float16, torch.float64):
            with pytest.raises(TypeError, match="expects fp32"):
                f(x.to(dt))


# ---- GPU: the table ------------------------------------------------------------------------------------------------------
WORST = {}


def _check_case(case, policy):
    r64, r32 = run_reference(case, F64), run_reference(case, torch.float32)
    for nc in (False, True):
        got = run_gpu(case, nc)
        assert set(got) == set(r64), (sorted(got), sorted(r64))
        for key in sorted(r64):
            assert tuple(got[key].shape) == tuple(r64[key].shape), (key, tuple(got[key].shape), tuple(r64[key].shape))
            tag = f"{case.id}{'-' + policy if policy else ''} [{'non-contiguous' if nc else 'contiguous'}] {key}"
            if case.is_exact(key):
                same = torch.equal(got[key], r32[key])
                print(f"{tag}: bit-exact {same}")
                assert same, f"{tag}: differs from the float32 CPU result at {(got[key] != r32[key]).nonzero()[:4].tolist()}"
                continue
            e_gpu, e32 = err(got[key], r64[key]), err(r32[key], r64[key])
            if case.kind == "conv":
                is_par = key.startswith("d") and key[1:] not in case.acts
                bound = CONV_LIMITS[policy][1 if is_par else 0]
            else:
                bound = 4 * e32 + FLOOR
            fam = case.family + (f" {policy}" if policy else "")
            WORST[fam] = max(WORST.get(fam, 0.0), e_gpu / bound)
            print(f"{tag}: e_gpu {e_gpu:.2e}  e_ref32 {e32:.2e}  bound {bound:.2e}  ratio {e_gpu / bound:.2f}")
            if not e_gpu <= bound:
                d = (got[key].double() - r64[key]).abs()
                at = tuple(int(i) for i in (d == d.max()).nonzero()[0]) if d.numel() else ()
                raise AssertionError(f"{tag}: e_gpu {e_gpu:.3e} > {bound:.3e} (e_ref32 {e32:.3e}); worst element {at}: got {got[key][at].item():.8g}, "
                                     f"float64 {r64[key][at].item():.8g}")


@pytest.mark.parametrize("case,policy", _params())
def test_op_vs_fp64(case, policy):
    from tpgsr_amd import kernels as K
    prev = K.POLICY
    if policy:
        K.set_conv_prec(policy)
    try:
        _check_case(case, policy)
    finally:
        K.set_conv_prec(prev)


@pytest.mark.gpu
def test_zz_report_worst_ratios():
    """prints the worst e_gpu / bound per family seen by this run (the module docstring's OBSERVED line is a copy of it)"""
    for fam in sorted(WORST):
        print(f"worst e_gpu / bound  {fam:32s} {WORST[fam]:.3f}")


# ---- GPU: what the table cannot express ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(1, 26), (16, 64), (8, 8), (3, 50), (1, 1)])
def test_bilinear_backward_is_the_adjoint(H, W):
    """<y, g> == <x, dx> in float64 of the GPU's own results, relative to sum |y g|: the backward kernel is the exact transpose of the forward"""
    from tpgsr_amd import functional as Fh
    for OH, OW in [(16, 64), (32, 64), (1, 1), (2, 13), (H, W)]:
        g = _gen("adjoint", H, W, OH, OW)
        x = torch.randn(2, H, W, 4, generator=g).to(DEV).requires_grad_(True)
        y = Fh.interpolate_bilinear(x, (OH, OW))
        gy = torch.randn(y.shape, generator=g).to(DEV)
        y.backward(gy)
        a, b = (y.detach().double() * gy.double()).sum().item(), (x.detach().double() * x.grad.double()).sum().item()
        scale = (y.detach().double() * gy.double()).abs().sum().item()
        print(f"bilinear {H}x{W} -> {OH}x{OW}: <y, g> {a:.9g}  <x, dx> {b:.9g}  |diff| / sum|y g| {abs(a - b) / scale:.2e}")
        assert abs(a - b) <= 1e-5 * scale


TIES = [("2x2s2-even", (2, 6, 10, 8), (2, 2), (2, 2), (0, 0)), ("2x2s2-odd", (2, 5, 9, 8), (2, 2), (2, 2), (0, 0)), ("2x2s2x1p0x1", (2, 4, 9, 8), (2, 2), (2, 1), (0, 1)),
        ("3x3s2p1", (2, 7, 9, 4), (3, 3), (2, 2), (1, 1)), ("2x2s2-C3", (1, 6, 10, 3), (2, 2), (2, 2), (0, 0))]


@pytest.mark.gpu
@pytest.mark.parametrize("name,shape,k,s,p", TIES, ids=[t[0] for t in TIES])
def test_max_pool_ties_go_to_the_first_maximum(name, shape, k, s, p):
    """windows with equal maxima -- a post-ReLU map quantised to steps of 0.5, with an all-zero region (what the OPT feature extractor feeds
    its pools): ATen routes the whole gradient to the first maximal element in window scan order; the same element-wise, and the
    gradient is conserved (per window where the windows do not overlap, per image and channel where they do)"""
    from tpgsr_amd import functional as Fh
    g = _gen("ties", name)
    x = torch.relu((torch.randn(*shape, generator=g) * 2).round() / 2)
    x[:, : shape[1] // 2, : shape[2] // 2] = 0.0
    xr = _nhwc(x).double().requires_grad_(True)
    yr = F.max_pool2d(xr, k, s, p)
    gy = torch.randn(yr.shape, generator=g)
    yr.backward(gy.double())
    ref = _nchw(xr.grad)
    xd = x.to(DEV).requires_grad_(True)
    yd = Fh.max_pool2d(xd, k, s, p)
    yd.backward(_nchw(gy).to(DEV).contiguous())
    got = xd.grad.cpu()
    assert torch.equal(yd.detach().cpu(), _nchw(yr.detach()).float())
    assert torch.equal(got != 0, ref != 0), f"gradient routed elsewhere at {((got != 0) != (ref != 0)).nonzero()[:4].tolist()}"
    e = err(got, ref)
    print(f"max-pool ties {name}: e_gpu {e:.2e}")
    assert e <= FLOOR
    if k == s and p == (0, 0):
        OH, OW = yr.shape[2:]
        win = got[:, : OH * k[0], : OW * k[1]].reshape(shape[0], OH, k[0], OW, k[1], shape[3]).sum((2, 4))
        assert torch.equal(win, _nchw(gy)) and got[:, OH * k[0]:].abs().sum() == 0 and got[:, :, OW * k[1]:].abs().sum() == 0
    tot, gt = got.double().sum((1, 2)), _nchw(gy).double().sum((1, 2))
    assert (tot - gt).abs().max() <= 1e-6 * _nchw(gy).double().abs().sum((1, 2)).max()


@pytest.mark.gpu
def test_refusals_come_from_the_host():
    """every 'raises' case of the table: refused before a launch, with a message that names the limit"""
    from tpgsr_amd import functional as Fh
    from tpgsr_amd._lib import TpgsrKernelError
    g = _gen("refusals")
    x = torch.randn(2, 4, 6, 8, generator=g).to(DEV)
    with pytest.raises(ValueError, match="input has 8 channels, weight expects 4"):
        Fh.conv2d(x, torch.randn(16, 4, 3, 3, device=DEV), padding=1)
    with pytest.raises(ValueError, match="empty output"):
        Fh.conv2d(x[:, :1], torch.randn(16, 8, 2, 2, device=DEV))
    for f in (Fh.relu, Fh.mish, Fh.tanh):
        with pytest.raises(ValueError, match="multiple of 4"):
            f(x[:, :3, :3, :3])
    with pytest.raises(TpgsrKernelError, match="multiple of 4"):
        Fh.prelu(x[:, :3, :3, :3], torch.ones(1, device=DEV))
    with pytest.raises(ValueError, match="add"):
        Fh.add(x, x[:, :3])
    with pytest.raises(ValueError, match="leading dimensions differ"):
        Fh.cat([x, x[:, :3]])
    with pytest.raises(TpgsrKernelError, match="C must be 1, 3 or 4"):
        Fh.grid_sample(x[..., :2], torch.zeros(2, 3, 3, 2, device=DEV), (3, 3))
    with pytest.raises(RuntimeError, match="evaluation path"):
        p = {k: v.to(DEV) for k, v in _rnn_params(g, 64, 32, 4).items()}
        Fh.bilstm_eval(torch.randn(2, 5, 64, device=DEV).requires_grad_(True), *[p[n] for n in _GRU_NAMES])
    with pytest.raises(ValueError, match="PackedLinear: out must be"):
        Fh.PackedLinear(torch.randn(8, 8, device=DEV))(x, out=torch.empty(5, 8, device=DEV))
    p = {k: v.to(DEV) for k, v in _rnn_params(g, 64, 16, 3).items()}
    with pytest.raises(NotImplementedError, match="hidden size 32"):
        Fh.bigru(torch.randn(1, 2, 3, 64, device=DEV), _gru_holder(p), 0)
    # BatchNorm: the backward of an eval-mode call; a channel count the vector backward kernels do not take
    d = {"gamma": torch.ones(8, device=DEV).requires_grad_(True), "beta": torch.zeros(8, device=DEV).requires_grad_(True), "rm": torch.zeros(8, device=DEV),
         "rv": torch.ones(8, device=DEV)}
    y = Fh.batch_norm(x.clone().requires_grad_(True), _bn_holder(d), False)
    with pytest.raises(RuntimeError, match="eval-mode BatchNorm"):
        y.sum().backward()
    d6 = {"gamma": torch.ones(6, device=DEV).requires_grad_(True), "beta": torch.zeros(6, device=DEV).requires_grad_(True), "rm": torch.zeros(6, device=DEV),
          "rv": torch.ones(6, device=DEV)}
    with pytest.raises(ValueError, match="multiple of 4"):
        Fh.batch_norm(x[..., :6].contiguous().requires_grad_(True), _bn_holder(d6), True)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_subsample_identity_returns_its_argument():
    from tpgsr_amd import functional as Fh
    x = torch.randn(1, 3, 3, 4, device=DEV)
    assert Fh.subsample(x, 1, 1) is x


@pytest.mark.gpu
@pytest.mark.parametrize("policy", ["x3", "x2"])
def test_gradient_sinks_accumulate(policy):
    """functional.GRAD_SINK: a convolution's weight + bias and a BatchNorm's gamma + beta accumulate their gradients into the sink buffers over
    two backward passes (the sum of both), autograd receives None for them, the convolution's `wscale` factor is applied"""
    from tpgsr_amd import functional as Fh, kernels as K
    g = _gen("sinks")
    ws = 0.5
    x1, x2 = torch.randn(2, 5, 7, 8, generator=g), torch.randn(2, 5, 7, 8, generator=g)
    w, b = torch.randn(16, 8, 3, 3, generator=g) / math.sqrt(72), torch.randn(16, generator=g)
    gamma, beta = torch.rand(8, generator=g) + 0.5, torch.randn(8, generator=g) * 0.3
    gy, gx = torch.randn(2, 5, 7, 16, generator=g), torch.randn(2, 5, 7, 8, generator=g)
    ref = {k: v.double().requires_grad_(True) for k, v in dict(w=w, b=b, gamma=gamma, beta=beta).items()}
    for x in (x1, x2):
        F.conv2d(_nhwc(x).double(), ref["w"] * ws, ref["b"], padding=1).backward(_nhwc(gy).double())
        F.batch_norm(_nhwc(x).double(), None, None, ref["gamma"], ref["beta"], True, 0.1, 1e-5).backward(_nhwc(gx).double())
    dev = {k: v.to(DEV).requires_grad_(True) for k, v in dict(w=w, b=b, gamma=gamma, beta=beta).items()}
    sinks = {k: torch.zeros_like(v.detach()) for k, v in dev.items()}
    prev = K.POLICY
    K.set_conv_prec(policy)
    try:
        with Fh.grad_sinks({dev[k].data_ptr(): sinks[k] for k in dev}):
            for x in (x1, x2):
                bn = types.SimpleNamespace(weight=dev["gamma"], bias=dev["beta"], running_mean=torch.zeros(8, device=DEV), running_var=torch.ones(8, device=DEV),
                                           momentum=0.1, eps=1e-5, num_batches_tracked=torch.tensor(0))
                xd = x.to(DEV).requires_grad_(True)
                Fh.conv2d(xd, dev["w"], dev["b"], padding=1, wscale=ws).backward(gy.to(DEV))
                Fh.batch_norm(xd, bn, True).backward(gx.to(DEV))
            torch.cuda.synchronize()
    finally:
        K.set_conv_prec(prev)
    assert all(v.grad is None for v in dev.values())
    for k in dev:
        e = err(sinks[k].cpu(), ref[k].grad)
        bound = CONV_LIMITS[policy][1]
        print(f"gradient sink {policy} {k}: e_gpu {e:.2e} (bound {bound:.0e})")
        assert e <= bound


# ---- gradient sinks, operator by operator ------------------------------------------------------------------------------------------------
def _sink_prelu(g):
    P = {"alpha": torch.full((1,), 0.25)}
    xs = [_away(torch.randn(1, 3, 5, 8, generator=g)) for _ in range(2)]
    return P, xs, (lambda x, p: F.prelu(x, p["alpha"])), (lambda Fh, x, p: Fh.prelu(x, p["alpha"])), None


def _sink_tconv(form, C):
    def make(g):
        P = {"w": torch.randn(C, C, 4, 4, generator=g) / math.sqrt(4 * C)}
        xs = [torch.randn(1, 3, 5, C, generator=g) for _ in range(2)]
        ref = lambda x, p: _nchw(F.conv_transpose2d(_nhwc(x), p["w"], stride=2, padding=1))
        return P, xs, ref, (lambda Fh, x, p: Fh.conv_transpose2d_k4s2(x, p["w"], form=form)), None
    return make


def _sink_dense(g, nf=8, gc=4, slope=0.2, res_scale=0.2):
    P = {}
    for k in range(5):
        cin, cout = nf + k * gc, (nf if k == 4 else gc)
        P[f"w{k}"], P[f"b{k}"] = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin), torch.randn(cout, generator=g) * 0.3
    xs = [torch.randn(1, 3, 5, nf, generator=g) for _ in range(2)]

    def pre(x, p):          # the pre-activations of the four LeakyReLUs, then the block's output
        cur, out = _nhwc(x), []
        for k in range(4):
            out.append(F.conv2d(cur, p[f"w{k}"], p[f"b{k}"], padding=1))
            cur = torch.cat([cur, F.leaky_relu(out[-1], slope)], 1)
        return out, _nchw(res_scale * F.conv2d(cur, p["w4"], p["b4"], padding=1) + _nhwc(x))
    gpu = lambda Fh, x, p: Fh.dense_block(x, [p[f"w{k}"] for k in range(5)], [p[f"b{k}"] for k in range(5)], slope, res_scale, form="inplace")
    return P, xs, (lambda x, p: pre(x, p)[1]), gpu, (lambda x, p: min(float(t.abs().min()) for t in pre(x, p)[0]))


def _sink_res(g, C=8, res_scale=0.1):
    P = {"w1": torch.randn(C, C, 3, 3, generator=g) / math.sqrt(9 * C), "w2": torch.randn(C, C, 3, 3, generator=g) / math.sqrt(9 * C)}
    xs = [torch.randn(1, 3, 5, C, generator=g) for _ in range(2)]
    pre = lambda x, p: F.conv2d(_nhwc(x), p["w1"], padding=1)
    ref = lambda x, p: _nchw(res_scale * F.conv2d(F.relu(pre(x, p)), p["w2"], padding=1) + _nhwc(x))
    return P, xs, ref, (lambda Fh, x, p: Fh.res_block(x, p["w1"], p["w2"], res_scale, form="fused")), (lambda x, p: float(pre(x, p).abs().min()))


def _sink_bigru(U, axis):
    def make(g):
        P = _rnn_params(g, 64, U, 3)
        xs = [torch.randn(1, 2, 5, 64, generator=g) for _ in range(2)]

        def ref(x, p):
            N, H, W, Cin = x.shape
            if axis == 0:
                return _rnn_ref(torch.nn.GRU, x.reshape(N * H, W, Cin), p, U).reshape(N, H, W, 2 * U)
            return _rnn_ref(torch.nn.GRU, x.permute(0, 2, 1, 3).reshape(N * W, H, Cin), p, U).reshape(N, W, H, 2 * U).permute(0, 2, 1, 3)
        return P, xs, ref, (lambda Fh, x, p: Fh.bigru(x, _gru_holder(p), axis)), None
    return make


# id -> (case builder, policy, rule of the bound: "conv" = CONV_LIMITS[policy][1], "arith" = 4 * e_ref32 + 4 * 2^-24)
SINK_OPS = {"prelu": (_sink_prelu, "x3", "arith"),
            "tconv_k4s2-direct-3to3": (_sink_tconv("direct", 3), "x3", "conv"),
            "tconv_k4s2-subpixel-64to64": (_sink_tconv("subpixel", 64), "x3", "conv"),
            "dense_block-inplace-nf8-gc4": (_sink_dense, "x3", "conv"),
            "res_block-fused-C8-x3": (_sink_res, "x3", "conv"),
            "res_block-fused-C8-f32": (_sink_res, "f32", "arith"),
            **{f"bigru-U{U}-axis{a}": (_sink_bigru(U, a), "x3", "conv") for U in (32, 64) for a in (0, 1)}}


def _sink_reference(name):
    """the first seed whose case keeps MARGIN from the kinks of its activations -> (parameters, inputs, upstream gradients, d parameter of the
    two passes summed in float64 and in float32 on the CPU, the GPU operator)"""
    make = SINK_OPS[name][0]
    for seed in range(32):
        P, xs, ref, gpu, margin = make(_gen("sink-op", name, seed))
        if margin is not None and min(margin(x.double(), {k: v.double() for k, v in P.items()}) for x in xs) < MARGIN:
            continue
        g = _gen("sink-op", name, seed, "upstream")
        gys, sums = None, {}
        for dtype in (F64, torch.float32):
            p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in P.items()}
            ys = [ref(x.to(dtype), p) for x in xs]
            gys = gys or [torch.randn(y.shape, generator=g) for y in ys]
            torch.autograd.backward(ys, [gy.to(dtype) for gy in gys])
            sums[dtype] = {k: v.grad for k, v in p.items()}
        return P, xs, gys, sums[F64], sums[torch.float32], gpu
    raise AssertionError(f"{name}: no seed keeps the margin")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SINK_OPS))
def test_gradient_sinks_accumulate_per_operator(name):
    """The operators test_gradient_sinks_accumulate does not reach, at the smallest shapes of their own cases.  Per operator: (1) ONE backward
    pass into zero-filled sinks gives, bit for bit, the gradients the same operator hands autograd without sinks (0 + g is exact, the kernels
    are the same), and autograd receives None; (2) a second pass, on another input, into the same sinks gives the float64 reference of the
    SUM of both gradients within the bound this file uses for that operator's parameter gradients -- CONV_LIMITS[policy][1] for the
    operators on the matrix cores and the direct convolution kernels under "x3"; the `arith` rule (4 * e_ref32 + 4 * 2^-24, e_ref32 from
    the float32 CPU run of the same two passes) for PReLU and for the plain-fp32 kernels of policy "f32", which has no CONV_LIMITS entry.
    (1) also holds on d97b637, the last commit with a sink lookup per operator, for every operator here that sank there -- all but bigru."""
    from tpgsr_amd import functional as Fh, kernels as K
    _, policy, rule = SINK_OPS[name]
    P, xs, gys, ref64, ref32, gpu = _sink_reference(name)

    def backward(i, p):
        gpu(Fh, xs[i].to(DEV).requires_grad_(True), p).backward(gys[i].to(DEV))
        torch.cuda.synchronize()
    with K.policy(policy):
        eager = {k: v.to(DEV).requires_grad_(True) for k, v in P.items()}
        backward(0, eager)
        dev = {k: v.to(DEV).requires_grad_(True) for k, v in P.items()}
        sinks = {k: torch.zeros_like(v.detach()) for k, v in dev.items()}
        with Fh.grad_sinks({dev[k].data_ptr(): sinks[k] for k in dev}):
            backward(0, dev)
            first = {k: v.clone() for k, v in sinks.items()}
            backward(1, dev)
    assert all(v.grad is None for v in dev.values()), [k for k, v in dev.items() if v.grad is not None]
    for k in P:
        assert eager[k].grad is not None and torch.equal(first[k], eager[k].grad), f"{name} {k}: one pass into a zero sink is not the eager gradient"
        e = err(sinks[k].cpu(), ref64[k])
        bound = CONV_LIMITS[policy][1] if rule == "conv" else 4 * err(ref32[k], ref64[k]) + FLOOR
        print(f"gradient sink {name} {k}: e_gpu {e:.2e} (bound {bound:.2e})")
        assert e <= bound, (name, k, e, bound)
