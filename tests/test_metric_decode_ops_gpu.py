"""The kernels evaluation is judged by and the small kernels around the recognisers -- PSNR, SSIM and its gradient, CTC greedy decode
(csrc/metrics.hip), the bicubic / strip resamplers and their adjoints (csrc/crnn.hip, csrc/aster.hip, csrc/elementwise.hip), the ASTER
decoder-step kernels (csrc/aster.hip) -- against stock PyTorch on the CPU in float64, over the sizes and edges their single fixtures and the
whole-network tests leave out.

Method and error rule: tests/kernel_table.py (the `arith` rule of tests/test_functional_ops_gpu.py; for scalars e_ref32 is the maximum over 8
seeds; on top, the limits the fixture tests assert: PSNR 1e-4 dB, SSIM value 2e-6 absolute and its gradient 2e-5 (test_ssim_loss_gpu.py)).

References:
  psnr / ssim      the formulas in the comments above psnr_partial_kernel / ssim_partial_kernel, F.conv2d(..., padding=KS // 2, groups=C);
                   ssim_bwd against autograd of mult * coef * ssim_map.sum(); the channels >= 3 of `da` keep their prefill bit for bit, with
                   accumulate=1 the first three hold prefill + gradient.  One window is NOT symmetric: the adjoint must flip it.
  greedy decode, softmax_max ids, embed_concat      exact, against a first-maximum arg-max written with comparisons and plain indexing.
  bicubic          F.interpolate(mode='bicubic', align_corners=False); bicubic_gray = 0.299 R + 0.587 G + 0.114 B of it; the backward against
                   autograd AND as the adjoint <fwd(x), g> == <x, bwd(g)> (float64 accumulation of the GPU's own results).
  strip resample   act(scale * x + shift) resampled along W by F.interpolate(mode='bilinear', align_corners=True); hsum: sum over H.
  attention, gru_cell      the three-line formulas in the kernels' comments.

softmax_max on a row with no finite maximum (all -inf, or NaN): the kernel leaves ids = INT_MAX and a NaN score (its scan never finds
`v > -inf`); the decode loop's next embed_concat clamps that id to V - 1.  test_softmax_max_row_without_a_maximum pins it; the kernel's
comment says so.

Observed on an MI355X: worst e_gpu / bound per family (test_zz_report_worst_ratios prints it; 0.25 = as accurate as float32 PyTorch on
the CPU):
  psnr 0.11, ssim 0.61, bicubic_gray 0.31, bicubic_resize 0.36, strip_resample 0.29, hsum 0.18, aster_attention 0.69, gru_cell 0.14,
  softmax_max 0.17; ctc_greedy_decode, embed_concat, softmax_max's ids and the untouched channels of ssim_bwd are bit-exact.
No family needs more than 4x, with one stated addition: the float32 floor of the SSIM gradient is taken relative to the three addends the
kernel sums (`_ssim_cancellation` has the derivation; without it the 1x1 window sits at 1.04, with the float32 CPU gradient itself at 7e-7).
"""
import math

import pytest
import torch
import torch.nn.functional as F

from kernel_table import DEV, F64, FLOOR, MARGIN, KCase, _gen, check_case, check_well_posed, err

FAMILY_KERNELS = {
    "psnr": {"psnr"}, "ssim": {"ssim", "ssim_bwd"}, "ctc_greedy_decode": {"ctc_greedy_decode"},
    "bicubic_gray": {"bicubic_gray_fwd", "bicubic_gray_bwd"}, "bicubic_resize": {"bicubic_resize"},
    "strip_resample": {"strip_resample_fwd", "strip_resample_bwd"}, "hsum": {"hsum"},
    "aster_attention": {"aster_attention"}, "embed_concat": {"embed_concat"}, "gru_cell": {"gru_cell"}, "softmax_max": {"softmax_max"},
}
NAMED_IN_THE_ISSUE = {"ssim", "ssim_bwd", "psnr", "ctc_greedy_decode", "bicubic_gray_fwd", "bicubic_gray_bwd", "bicubic_resize", "strip_resample_fwd",
                      "strip_resample_bwd", "hsum", "aster_attention", "embed_concat", "gru_cell", "softmax_max"}
ACT = {"none": 0, "relu": 1, "mish": 2, "tanh": 3}


def K():
    from tpgsr_amd import kernels
    return kernels


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _margin(value, what, m=MARGIN):
    assert value >= m, f"{what}: margin {value:.3e} < {m:.0e}"


# ---- PSNR / SSIM ------------------------------------------------------------------------------------------------------------
def _img_make(shape, seed):
    g = _gen("images", shape, seed)
    a = torch.rand(*shape, generator=g)
    return {"a": a, "b": (a + 0.1 * torch.randn(*shape, generator=g)).clamp(0, 1), "pre": torch.randn(*shape, generator=g), "coef": torch.rand(1, generator=g) + 0.5}


def _psnr_ref(d):
    a, b = d["a"][:, :3], d["b"][:, :3]
    mse = ((a * 255 - b * 255) ** 2).mean()
    return {"psnr": (20 * torch.log10(255.0 / torch.sqrt(mse))).reshape(())}


def _psnr_gpu(d, nblk):
    N, C, H, W = d["a"].shape
    part, out = torch.full((nblk,), float("nan"), dtype=F64, device=DEV), _nan(1)
    K().psnr(d["a"], d["b"], N, C, H, W, part, nblk, out)
    return {"psnr": out.reshape(())}


def _window(kind):
    if kind.startswith("gauss"):
        ks = int(kind[5:])
        g = torch.tensor([math.exp(-(x - ks // 2) ** 2 / (2 * 1.5 ** 2)) for x in range(ks)], dtype=F64)
        g = g / g.sum()
        return (g[:, None] * g[None, :]).float()
    if kind == "one":
        return torch.ones(1, 1)
    ks = int(kind[4:])                      # "skew5": positive, normalised, symmetric in neither direction
    w = torch.rand(ks, ks, generator=_gen("window", kind)) + 0.1 * torch.arange(ks * ks).view(ks, ks)
    return (w / w.sum()).float()


def _ssim_map(a, b, win, aa=None, ab=None):
    Cc, KS = a.shape[1], win.shape[0]
    w = win.to(a.dtype).view(1, 1, KS, KS).expand(Cc, 1, KS, KS).contiguous()
    conv = lambda x: F.conv2d(x, w, padding=KS // 2, groups=Cc)
    mu1, mu2 = conv(a), conv(b)
    s11, s22, s12 = conv(a * a if aa is None else aa) - mu1 * mu1, conv(b * b) - mu2 * mu2, conv(a * b if ab is None else ab) - mu1 * mu2
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    return ((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s11 + s22 + c2))


def _ssim_ref(d, win, mult, use_coef, accumulate):
    a = d["a"].clone().requires_grad_(True)
    Cc = min(a.shape[1], 3)
    smap = _ssim_map(a[:, :Cc], d["b"][:, :Cc], win)
    k = mult * (d["coef"][0] if use_coef else 1.0)
    (k * smap.sum()).backward()
    da = a.grad[:, :Cc]
    return {"ssim": smap.mean().detach().reshape(()), "da": da + d["pre"][:, :Cc] if accumulate else da, "da_rest": d["pre"][:, Cc:]}


def _ssim_cancellation(d64, win):
    """The kernel forms d S / d a as the sum of three separately rounded float32 addends, (w * G0) + 2 a (w * G1) + b (w * G2) (the comment above
    ssim_grad_maps_kernel): each carries 2^-24 of ITS OWN size, and with a small window their sum is far smaller than they are (for a 1x1
    window the variances vanish identically and the addends are of size S / C2 ~ 1e3).  The float32 floor of the rule, 4 * 2^-24, is
    therefore taken relative to the addends: extra = 4 * 2^-24 * (max (|A0| + |A1| + |A2|) / max |A0 + A1 + A2| - 1), from float64 autograd
    with a, a^2 and a b as separate leaves."""
    Cc = min(d64["a"].shape[1], 3)
    a, b = d64["a"][:, :Cc], d64["b"][:, :Cc]
    a1, aa, ab = a.clone().requires_grad_(True), (a * a).requires_grad_(True), (a * b).requires_grad_(True)
    _ssim_map(a1, b, win, aa, ab).sum().backward()
    adds = [a1.grad, 2 * a * aa.grad, b * ab.grad]
    return FLOOR * (sum(x.abs() for x in adds).max().item() / sum(adds).abs().max().item() - 1)


def _ssim_gpu(d, win, mult, use_coef, accumulate, nblk):
    k = K()
    N, C, H, W = d["a"].shape
    Cc, KS = min(C, 3), win.shape[0]
    wd = win.to(DEV).contiguous()
    part, out = torch.full((nblk,), float("nan"), dtype=F64, device=DEV), _nan(1)
    k.ssim(d["a"], d["b"], wd, KS, N, C, H, W, part, nblk, out)
    da, gm = d["pre"].clone(), _nan(3 * N * Cc * H * W)
    k.ssim_bwd(d["a"], d["b"], wd, KS, N, C, H, W, gm, d["coef"] if use_coef else None, mult, da, accumulate)
    return {"ssim": out.reshape(()), "da": da[:, :Cc], "da_rest": da[:, Cc:]}


SSIM = [
    # name, (N, Ctot, H, W), window, mult, coef tensor, accumulate, nblk
    ("C4-16x64-gauss11", (2, 4, 16, 64), "gauss11", -10.0 / (2 * 3 * 16 * 64), False, True, 64),
    ("C3-7x9-smaller-than-the-window", (2, 3, 7, 9), "gauss11", 1.0 / (2 * 3 * 7 * 9), True, False, 64),
    ("C1-N1-5x33", (1, 1, 5, 33), "gauss11", 1.0, True, True, 1),
    ("C2-12x10-gauss3", (3, 2, 12, 10), "gauss3", 0.01, False, False, 4),
    ("C4-9x11-window1", (2, 4, 9, 11), "one", 0.02, True, True, 64),
    ("C3-40x36-gauss33", (1, 3, 40, 36), "gauss33", 1e-3, True, False, 64),
    ("C4-13x17-skew5", (2, 4, 13, 17), "skew5", 0.01, True, False, 16),
    ("C3-3x4-skew3", (1, 3, 3, 4), "skew3", 1.0, False, True, 2),
    ("C3-300x400-gauss3-grid-stride", (3, 3, 300, 400), "gauss3", 1e-5, True, False, 256),
]


def _metric_cases():
    out = []
    for shape, nblk in [((2, 4, 16, 64), 64), ((1, 1, 3, 5), 1), ((3, 2, 7, 9), 64), ((2, 3, 32, 128), 7), ((1, 4, 1, 1), 4)]:
        out.append(KCase("psnr", f"{'x'.join(map(str, shape))}-nblk{nblk}", lambda seed, s=shape: _img_make(s, seed), _psnr_ref, lambda d, nblk=nblk: _psnr_gpu(d, nblk),
                         scalars=["psnr"], abs_caps={"psnr": 1e-4}))
    for name, shape, wk, mult, use_coef, acc, nblk in SSIM:
        win = _window(wk)
        out.append(KCase("ssim", name, lambda seed, s=shape: _img_make(s, seed), lambda d, a=(win, mult, use_coef, acc): _ssim_ref(d, *a),
                         lambda d, a=(win, mult, use_coef, acc, nblk): _ssim_gpu(d, *a), scalars=["ssim"], exact=["da_rest"], caps={"da": 2e-5}, abs_caps={"ssim": 2e-6},
                         extra={"da": lambda d64, win=win: _ssim_cancellation(d64, win)}))
    return out


# ---- greedy decode ---------------------------------------------------------------------------------------------------------
def _first_argmax(x):
    """index of the FIRST maximum along the last axis, by comparisons only"""
    C = x.shape[-1]
    hit = x == x.max(-1, keepdim=True).values
    return torch.where(hit, torch.arange(C).expand_as(x), torch.full_like(x, C, dtype=torch.long)).min(-1).values


def _greedy_ref(d):
    x = d["logits"]
    N, T, _C = x.shape
    am = _first_argmax(x).tolist()
    labels, lengths = torch.full((N, T), -1, dtype=torch.int32), torch.zeros(N, dtype=torch.int32)
    for n in range(N):
        last, out = -1, []
        for i in am[n]:
            if i != last:
                if i != 0:
                    out.append(i)
                    last = i
                else:
                    last = -1
        labels[n, :len(out)] = torch.tensor(out, dtype=torch.int32)
        lengths[n] = len(out)
    return {"labels": labels, "lengths": lengths}


def _greedy_gpu(d):
    N, T, C = d["logits"].shape
    labels, lengths = torch.full((N, T), -7, dtype=torch.int32, device=DEV), torch.full((N,), -7, dtype=torch.int32, device=DEV)
    K().ctc_greedy_decode(d["logits"], N, T, C, labels, lengths)
    return {"labels": labels, "lengths": lengths}


def _greedy_make(N, T, C, kind, seed):
    g = _gen("greedy", N, T, C, kind, seed)
    x = torch.randn(N, T, C, generator=g)
    if kind == "ties":                  # logits in steps of 0.5: several equal maxima in most rows
        x = (x * 1.5).round() / 2
    elif kind == "crafted":             # sample 0 all blank, sample 1 "a-a" (two labels), sample 2 "aa" (one), sample 3 every class equal (blank wins)
        x = torch.zeros(N, T, C)
        x[0, :, 0] = 1.0
        a = min(3, C - 1)
        x[1, :, 0] = 1.0
        x[1, 0, a] = x[1, 2, a] = 2.0
        x[2, :, 0] = 1.0
        x[2, 0, a] = x[2, 1, a] = 2.0
    return {"logits": x}


def _greedy_cases():
    out = []
    for N, T, C, kind in [(3, 26, 37, "plain"), (4, 26, 37, "ties"), (4, 26, 37, "crafted"), (2, 1, 37, "plain"), (2, 1024, 37, "ties"), (3, 100, 37, "ties"),
                          (2, 65, 5, "ties"), (2, 7, 1, "plain"), (2, 64, 97, "plain")]:
        out.append(KCase("ctc_greedy_decode", f"T{T}-C{C}-{kind}", lambda seed, a=(N, T, C, kind): _greedy_make(*a, seed), _greedy_ref, _greedy_gpu,
                         exact=["labels", "lengths"]))
    return out


# ---- bicubic / strip resample / hsum ------------------------------------------------------------------------------------------
LUM = (0.299, 0.587, 0.114)
BICUBIC = [((16, 64), (32, 100)), ((32, 128), (32, 100)), ((40, 250), (32, 100)), ((32, 100), (32, 100)), ((1, 5), (4, 9)), ((3, 2), (5, 7)), ((2, 1), (3, 3)),
           ((7, 11), (32, 100)), ((9, 13), (3, 4))]


def _gray_ref(d, size):
    x = d["x"].clone().requires_grad_(True)
    y = F.interpolate(x[:, :3], size=size, mode="bicubic", align_corners=False)
    gray = LUM[0] * y[:, 0:1] + LUM[1] * y[:, 1:2] + LUM[2] * y[:, 2:3]
    (gray * d["g"]).sum().backward()
    return {"gray": gray.detach(), "dx": x.grad}


def _gray_gpu(d, size):
    k = K()
    N, C, H, W = d["x"].shape
    out, din = _nan(N, 1, *size), _nan(N, C, H, W)
    k.bicubic_gray_fwd(d["x"], N, C, H, W, size[0], size[1], out)
    k.bicubic_gray_bwd(d["g"], N, C, H, W, size[0], size[1], din)
    return {"gray": out, "dx": din}


def _resize_ref(d, size, C, scale, shift):
    y = F.interpolate(d["x"][:, :C], size=size, mode="bicubic", align_corners=False) * scale + shift
    return {"y": y.permute(0, 2, 3, 1)}


def _resize_gpu(d, size, C, scale, shift):
    N, Ctot, H, W = d["x"].shape
    out = _nan(N, size[0], size[1], C)
    K().bicubic_resize(d["x"], N, Ctot, C, H, W, size[0], size[1], scale, shift, out)
    return {"y": out}


STRIP = [
    # Win, Wout, C, act, affine
    (26, 64, 32, "none", False), (203, 64, 32, "relu", True), (5, 5, 5, "tanh", True), (1, 7, 4, "none", True), (7, 1, 4, "mish", False), (2, 9, 3, "mish", True),
    (64, 26, 8, "relu", True), (3, 2, 1, "none", False),
]


def _strip_make(N, Win, Wout, C, act, affine, seed):
    g = _gen("strip", Win, Wout, C, act, seed)
    sc, sh = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    z = torch.randn(N, Win, C, generator=g)
    if act == "relu":          # the pre-activation value stays 2e-3 clear of the kink
        z = torch.where(z.abs() < 2 * MARGIN, torch.full_like(z, 2 * MARGIN), z)
    d = {"x": (z - sh) / sc if affine else z, "g": torch.randn(N, Wout, C, generator=g)}
    if affine:
        d.update(scale=sc, shift=sh)
    return d


def _strip_pre(d):
    return d["x"] * d["scale"] + d["shift"] if "scale" in d else d["x"]


def _strip_ref(d, Wout, act):
    x = d["x"].clone().requires_grad_(True)
    z = _strip_pre({**d, "x": x})
    a = {"none": lambda t: t, "relu": F.relu, "mish": F.mish, "tanh": torch.tanh}[act](z)
    y = F.interpolate(a.permute(0, 2, 1).unsqueeze(2), size=(1, Wout), mode="bilinear", align_corners=True).squeeze(2).permute(0, 2, 1)
    (y * d["g"]).sum().backward()
    return {"y": y.detach(), "dx": x.grad}


def _strip_gpu(d, Wout, act):
    k = K()
    N, Win, C = d["x"].shape
    y, dz = _nan(N, Wout, C), _nan(N, Win, C)
    k.strip_resample_fwd(d["x"], d.get("scale"), d.get("shift"), ACT[act], N, Win, Wout, C, y)
    k.strip_resample_bwd(d["x"], d.get("scale"), d.get("shift"), ACT[act], d["g"], N, Win, Wout, C, dz)
    # dz is the gradient with respect to the pre-activation value scale * x + shift: the chain rule through the affine is the caller's
    return {"y": y, "dx": dz * d["scale"] if "scale" in d else dz}


def _hsum_ref(d, accumulate):
    s = d["d"].sum(1)
    return {"strip": s + d["pre"] if accumulate else s}


def _hsum_gpu(d, accumulate):
    N, H, W, C = d["d"].shape
    out = d["pre"].clone() if accumulate else _nan(N, W, C)
    K().hsum(d["d"], N, H, W, C, out, accumulate)
    return {"strip": out}


def _resample_cases():
    out = []
    for (H, W), size in BICUBIC:
        for Ctot in (3, 4):
            make = lambda seed, a=(H, W, size, Ctot): {"x": torch.rand(2, a[3], a[0], a[1], generator=_gen("bicubic", a, seed)),
                                                       "g": torch.randn(2, 1, *a[2], generator=_gen("bicubic-g", a, seed))}
            name = f"{H}x{W}-to-{size[0]}x{size[1]}-Ctot{Ctot}"
            out.append(KCase("bicubic_gray", name, make, lambda d, s=size: _gray_ref(d, s), lambda d, s=size: _gray_gpu(d, s)))
            C, scale, shift = (3, 2.0, -1.0) if Ctot == 4 else (Ctot, 1.0, 0.0)
            out.append(KCase("bicubic_resize", f"{name}-C{C}", make, lambda d, a=(size, C, scale, shift): _resize_ref(d, *a),
                             lambda d, a=(size, C, scale, shift): _resize_gpu(d, *a)))
    out.append(KCase("bicubic_resize", "5x6-to-32x100-C1-of-2", lambda seed: {"x": torch.rand(3, 2, 5, 6, generator=_gen("bicubic-c1", seed))},
                     lambda d: _resize_ref(d, (32, 100), 1, 0.5, 0.25), lambda d: _resize_gpu(d, (32, 100), 1, 0.5, 0.25)))
    for Win, Wout, C, act, affine in STRIP:
        margin = (lambda d64: _margin(_strip_pre(d64).abs().min().item(), "|scale x + shift| of a ReLU input")) if act == "relu" else None
        out.append(KCase("strip_resample", f"{Win}-to-{Wout}-C{C}-{act}{'-affine' if affine else ''}", lambda seed, a=(2, Win, Wout, C, act, affine): _strip_make(*a, seed),
                         lambda d, a=(Wout, act): _strip_ref(d, *a), lambda d, a=(Wout, act): _strip_gpu(d, *a), margin=margin))
    for N, H, W, C, acc in [(2, 1, 3, 4, False), (2, 7, 26, 32, True), (1, 8, 5, 4, False), (2, 9, 2, 2, True), (3, 16, 64, 32, False), (1, 17, 1, 4, True)]:
        out.append(KCase("hsum", f"H{H}-W{W}-C{C}{'-accumulate' if acc else ''}",
                         lambda seed, a=(N, H, W, C): {"d": torch.randn(*a, generator=_gen("hsum", a, seed)), "pre": torch.randn(a[0], a[2], a[3], generator=_gen("hsum-pre", a, seed))},
                         lambda d, acc=acc: _hsum_ref(d, acc), lambda d, acc=acc: _hsum_gpu(d, acc)))
    return out


# ---- ASTER decoder-step kernels -----------------------------------------------------------------------------------------------
def _attn_make(N, T, A, D, seed):
    g = _gen("attention", N, T, A, D, seed)
    return {"xproj": torch.randn(N, T, A, generator=g), "sproj": torch.randn(N, A, generator=g), "wv": torch.randn(A, generator=g) / math.sqrt(A),
            "bv": torch.randn(1, generator=g), "x": torch.randn(N, T, D, generator=g)}


def _attn_ref(d):
    v = torch.tanh(d["sproj"][:, None, :] + d["xproj"]) @ d["wv"] + d["bv"]
    alpha = torch.softmax(v, 1)
    return {"alpha": alpha, "context": (alpha[..., None] * d["x"]).sum(1)}


def _attn_gpu(d):
    N, T, A = d["xproj"].shape
    D = d["x"].shape[2]
    alpha, ctx = _nan(N, T), _nan(N, D)
    K().aster_attention(d["xproj"], d["sproj"], d["wv"], d["bv"], d["x"], N, T, A, D, alpha, ctx)
    return {"alpha": alpha, "context": ctx}


def _embed_make(N, V, E, D, seed):
    g = _gen("embed", N, V, E, D, seed)
    ids = torch.randint(0, V, (N,), generator=g, dtype=torch.int32)
    ids[0], ids[-1] = -3, V + 5          # inside the kernel's clamp
    if N > 2:
        ids[1] = V - 1
    return {"ids": ids, "emb": torch.randn(V, E, generator=g), "ctx": torch.randn(N, D, generator=g)}


def _embed_ref(d):
    V = d["emb"].shape[0]
    return {"out": torch.cat([d["emb"][d["ids"].long().clamp(0, V - 1)], d["ctx"]], 1)}


def _embed_gpu(d):
    (V, E), (N, D) = d["emb"].shape, d["ctx"].shape
    out = _nan(N, E + D)
    K().embed_concat(d["ids"], d["emb"], V, E, d["ctx"], D, N, out)
    return {"out": out}


def _gru_ref(d):
    gi, gh, h = d["gi"], d["gh"], d["h"]
    Hd = h.shape[1]
    r = torch.sigmoid(gi[:, :Hd] + gh[:, :Hd])
    z = torch.sigmoid(gi[:, Hd:2 * Hd] + gh[:, Hd:2 * Hd])
    n = torch.tanh(gi[:, 2 * Hd:] + r * gh[:, 2 * Hd:])
    return {"h": (1 - z) * n + z * h}


def _gru_gpu(d):
    N, Hd = d["h"].shape
    out = _nan(N, Hd)
    K().gru_cell(d["gi"], d["gh"], d["h"], N, Hd, out)
    return {"h": out}


def _top2_gap(x):
    t = x.topk(2, -1).values
    return (t[..., 0] - t[..., 1]).min().item()


def _smax_make(N, C, seed):
    for s in range(64):          # the first generator whose rows keep their two largest logits 2e-3 apart
        x = torch.randn(N, C, generator=_gen("softmax_max", N, C, seed, s)) * 3
        if C == 1 or _top2_gap(x.double()) >= 2 * MARGIN:
            break
    return {"logits": x}


def _smax_ref(d, ld, col, nxt):
    x = d["logits"]
    N = x.shape[0]
    ids, score = torch.full((N, ld), -7, dtype=torch.int32), torch.full((N, ld), -7.0, dtype=x.dtype)
    am = _first_argmax(x)
    ids[:, col], score[:, col] = am.int(), torch.softmax(x, -1).gather(1, am[:, None])[:, 0]
    res = {"ids": ids, "score": score}
    if nxt:
        res["ids_next"] = am.int()
    return res


def _smax_gpu(d, ld, col, nxt):
    N, C = d["logits"].shape
    ids, score = torch.full((N, ld), -7, dtype=torch.int32, device=DEV), torch.full((N, ld), -7.0, device=DEV)
    ids_next = torch.full((N,), -7, dtype=torch.int32, device=DEV) if nxt else None
    K().softmax_max(d["logits"], N, C, ids, score, ld, col, ids_next)
    res = {"ids": ids, "score": score}
    if nxt:
        res["ids_next"] = ids_next
    return res


def _aster_cases():
    out = []
    for N, T, A, D in [(2, 1, 64, 256), (3, 25, 256, 512), (1, 256, 100, 300), (2, 7, 3, 5), (2, 64, 65, 257), (1, 255, 256, 1)]:
        out.append(KCase("aster_attention", f"T{T}-A{A}-D{D}", lambda seed, a=(N, T, A, D): _attn_make(*a, seed), _attn_ref, _attn_gpu))
    for N, V, E, D in [(2, 97, 512, 512), (5, 3, 7, 1), (3, 1, 1, 9), (300, 97, 5, 3)]:
        out.append(KCase("embed_concat", f"N{N}-V{V}-E{E}-D{D}", lambda seed, a=(N, V, E, D): _embed_make(*a, seed), _embed_ref, _embed_gpu, exact=["out"]))
    for N, Hd in [(1, 1), (5, 256), (3, 100), (64, 7)]:
        out.append(KCase("gru_cell", f"N{N}-Hd{Hd}",
                         lambda seed, a=(N, Hd): dict(zip(("gi", "gh", "h"), (torch.randn(*s, generator=_gen("gru_cell", a, seed, i)) * 2
                                                                                for i, s in enumerate([(a[0], 3 * a[1]), (a[0], 3 * a[1]), a])))),
                         _gru_ref, _gru_gpu))
    for N, C, ld, col, nxt in [(3, 97, 25, 0, True), (2, 37, 4, 3, False), (4, 64, 1, 0, True), (2, 65, 3, 1, True), (1, 1, 2, 1, False), (2, 300, 5, 2, True)]:
        out.append(KCase("softmax_max", f"C{C}-ld{ld}-col{col}{'-next' if nxt else ''}", lambda seed, a=(N, C): _smax_make(*a, seed),
                         lambda d, a=(ld, col, nxt): _smax_ref(d, *a), lambda d, a=(ld, col, nxt): _smax_gpu(d, *a),
                         exact=["ids", "ids_next"] if nxt else ["ids"],
                         margin=(lambda d64: _margin(_top2_gap(d64["logits"]), "two largest logits of a row")) if C > 1 else None))
    return out


_CASES = None


def all_cases():
    global _CASES
    if _CASES is None:
        _CASES = _metric_cases() + _greedy_cases() + _resample_cases() + _aster_cases()
        ids = [c.id for c in _CASES]
        assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return _CASES


# ---- CPU: the table is well posed ------------------------------------------------------------------------------------------------
def test_case_table_is_well_posed():
    """Every case on the CPU: margins (ReLU kink of the strip's activation, arg-max gap of softmax_max), a finite float64 reference with
    every output and gradient, a finite e_ref32 (over 8 seeds for the scalars), inputs under 8 MB, the contract limits (greedy decode T <= 1024,
    attention T <= 256, window <= 33 and odd); the families cover every kernel the table of the issue names; one SSIM window is not symmetric."""
    cases = all_cases()
    assert {c.family for c in cases} == set(FAMILY_KERNELS)
    assert set().union(*FAMILY_KERNELS.values()) >= NAMED_IN_THE_ISSUE
    for c in cases:
        check_well_posed(c)
        if c.family == "ctc_greedy_decode":
            assert c.ins["logits"].shape[1] <= 1024
        if c.family == "aster_attention":
            assert c.ins["xproj"].shape[1] <= 256
    wins = {wk: _window(wk) for _n, _s, wk, *_r in SSIM}
    assert all(w.shape[0] % 2 == 1 and w.shape[0] <= 33 and abs(w.double().sum().item() - 1) < 1e-6 for w in wins.values())
    assert any(not torch.equal(w, w.flip(0)) and not torch.equal(w, w.flip(1)) and not torch.equal(w, w.t()) for w in wins.values())
    assert any(s[0] * min(s[1], 3) * s[2] * s[3] > 4096 * 256 for _n, s, *_r in SSIM)          # the grid-stride path of both backward kernels
    # the crafted greedy-decode rows say what their names say
    r = _greedy_ref(_greedy_make(4, 26, 37, "crafted", 0))
    assert r["lengths"].tolist() == [0, 2, 1, 0] and r["labels"][1, :3].tolist() == [3, 3, -1] and r["labels"][2, :2].tolist() == [3, -1]


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
WORST = {}


@pytest.mark.parametrize("case", [pytest.param(c, id=c.id, marks=pytest.mark.gpu) for c in all_cases()])
def test_kernel_vs_fp64(case):
    check_case(case, WORST)


def _dot(a, b):
    return (a.double() * b.double()).sum().item(), (a.double() * b.double()).abs().sum().item()


@pytest.mark.gpu
def test_backward_kernels_are_the_adjoints():
    """<fwd(x), g> == <x, bwd(g)> in float64 accumulation of the GPU's own results, relative to sum |fwd(x) g| (1e-5, the bound of
    test_functional_ops_gpu.py::test_bilinear_backward_is_the_adjoint): bicubic_gray, strip_resample (identity activation), hsum (the
    adjoint of broadcasting a strip over H)"""
    k = K()
    for (H, W), size in BICUBIC:
        for Ctot in (3, 4):
            g = _gen("adjoint-bicubic", H, W, size, Ctot)
            x, gy = torch.randn(2, Ctot, H, W, generator=g).to(DEV), torch.randn(2, 1, *size, generator=g).to(DEV)
            y, dx = _nan(2, 1, *size), _nan(2, Ctot, H, W)
            k.bicubic_gray_fwd(x, 2, Ctot, H, W, size[0], size[1], y)
            k.bicubic_gray_bwd(gy, 2, Ctot, H, W, size[0], size[1], dx)
            torch.cuda.synchronize()
            (a, scale), (b, _s) = _dot(y, gy), _dot(x, dx)
            print(f"bicubic_gray {H}x{W} -> {size} Ctot {Ctot}: <y, g> {a:.9g}  <x, dx> {b:.9g}  |diff| / sum|y g| {abs(a - b) / scale:.2e}")
            assert abs(a - b) <= 1e-5 * scale
            assert Ctot == 3 or torch.equal(dx[:, 3:], torch.zeros_like(dx[:, 3:]))            # the mask channel takes no gradient
    for Win, Wout, C, _act, _aff in STRIP:
        g = _gen("adjoint-strip", Win, Wout, C)
        x, gy = torch.randn(2, Win, C, generator=g).to(DEV), torch.randn(2, Wout, C, generator=g).to(DEV)
        y, dx = _nan(2, Wout, C), _nan(2, Win, C)
        k.strip_resample_fwd(x, None, None, 0, 2, Win, Wout, C, y)
        k.strip_resample_bwd(x, None, None, 0, gy, 2, Win, Wout, C, dx)
        torch.cuda.synchronize()
        (a, scale), (b, _s) = _dot(y, gy), _dot(x, dx)
        print(f"strip_resample {Win} -> {Wout} C {C}: <y, g> {a:.9g}  <x, dx> {b:.9g}  |diff| / sum|y g| {abs(a - b) / scale:.2e}")
        assert abs(a - b) <= 1e-5 * scale
    for N, H, W, C in [(2, 7, 26, 32), (1, 17, 1, 4), (2, 8, 3, 4)]:
        g = _gen("adjoint-hsum", N, H, W, C)
        s, d = torch.randn(N, W, C, generator=g).to(DEV), torch.randn(N, H, W, C, generator=g).to(DEV)
        out = _nan(N, W, C)
        k.hsum(d, N, H, W, C, out, False)
        torch.cuda.synchronize()
        (a, scale), (b, _s) = _dot(s[:, None].expand(N, H, W, C), d), _dot(s, out)
        assert abs(a - b) <= 1e-5 * scale


@pytest.mark.gpu
def test_softmax_max_ties_go_to_the_lowest_index():
    """equal maxima in different lanes (c, c + 1), in one lane's strided scan (c, c + 64), and in both; every class equal; the kernel's shuffle
    tree must keep the lowest index, as torch.max does"""
    k = K()
    rows = []
    for C in (37, 64, 65, 200):
        for pair in [(0, 1), (5, 6), (C - 2, C - 1), (3, C - 1), (1, 33), (31, 32)] + ([(2, 66), (2, 3, 66), (63, 64), (0, 64, 128)] if C > 128 else []) + \
                    ([(0, 64)] if C == 65 else []):
            x = -torch.rand(C, generator=_gen("smax-ties", C, pair)) - 0.5
            x[list(pair)] = 1.25
            rows.append((x, min(pair)))
        rows.append((torch.full((C,), 0.75), 0))
    for x, want in rows:
        C = x.numel()
        ids, score = torch.full((1, 1), -7, dtype=torch.int32, device=DEV), _nan(1, 1)
        k.softmax_max(x.view(1, C).to(DEV), 1, C, ids, score, 1, 0, None)
        torch.cuda.synchronize()
        assert int(ids.item()) == want == int(_first_argmax(x.view(1, C)).item()), (C, want, int(ids.item()))
        assert err(score.cpu().view(1), torch.softmax(x.double(), 0)[want].view(1)) <= 4 * 2.0 ** -23


@pytest.mark.gpu
def test_softmax_max_row_without_a_maximum():
    """a row of -inf (and a row of NaN): no `v > best` ever holds, so ids stays INT_MAX and the score is NaN; the other rows of the batch are
    untouched by it, and embed_concat clamps the id to V - 1 -- documented at the kernel"""
    k = K()
    x = torch.randn(3, 37, generator=_gen("smax-noinf"))
    x[1] = float("-inf")
    x[2, 5] = float("nan")          # a NaN compares false: the row's maximum is taken over the other classes
    ids, score, nxt = torch.full((3, 2), -7, dtype=torch.int32, device=DEV), torch.full((3, 2), -7.0, device=DEV), torch.full((3,), -7, dtype=torch.int32, device=DEV)
    k.softmax_max(x.to(DEV), 3, 37, ids, score, 2, 1, nxt)
    emb, ctx, out = torch.arange(10.0, device=DEV).view(5, 2), torch.zeros(3, 1, device=DEV), _nan(3, 3)
    k.embed_concat(nxt, emb, 5, 2, ctx, 1, 3, out)
    torch.cuda.synchronize()
    assert ids[:, 0].tolist() == [-7, -7, -7] and ids[0, 1].item() == int(_first_argmax(x[:1]).item())
    assert ids[1, 1].item() == 0x7FFFFFFF == nxt[1].item() and math.isnan(score[1, 1].item())
    y = x[2].clone()
    y[5] = float("-inf")
    assert ids[2, 1].item() == int(_first_argmax(y.view(1, -1)).item())
    assert out[1, :2].tolist() == [8.0, 9.0]


@pytest.mark.gpu
def test_argument_guards():
    """just past each limit of the contract: the library's own error, before any launch"""
    from tpgsr_amd._lib import TpgsrKernelError
    k = K()
    x = torch.zeros(4096, device=DEV)
    i32 = torch.zeros(4096, dtype=torch.int32, device=DEV)
    p64 = torch.zeros(4, dtype=F64, device=DEV)
    with pytest.raises(TpgsrKernelError, match="T <= 1024"):
        k.ctc_greedy_decode(x, 1, 1025, 2, i32, i32)
    with pytest.raises(TpgsrKernelError, match="T must be <= 256"):
        k.aster_attention(x, x, x, x, x, 1, 257, 2, 2, x, x)
    for ks in (35, 4):
        with pytest.raises(TpgsrKernelError, match="odd window <= 33"):
            k.ssim(x, x, x, ks, 1, 1, 4, 4, p64, 4, x)
        with pytest.raises(TpgsrKernelError, match="odd window <= 33"):
            k.ssim_bwd(x, x, x, ks, 1, 1, 4, 4, x, None, 1.0, x, False)
    with pytest.raises(TpgsrKernelError, match="bad arguments"):
        k.bicubic_gray_fwd(x, 1, 2, 4, 4, 4, 4, x)                      # Ctot < 3
    with pytest.raises(TpgsrKernelError, match="bad arguments"):
        k.bicubic_resize(x, 1, 2, 3, 4, 4, 4, 4, 1.0, 0.0, x)           # C > Ctot
    with pytest.raises(TpgsrKernelError, match="W C % 4 == 0"):
        k.hsum(x, 1, 2, 3, 1, x, False)
    with pytest.raises(TpgsrKernelError, match="bad arguments"):
        k.softmax_max(x, 1, 4, i32, x, 2, 2, None)                      # col == ld
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_zz_report_worst_ratios():
    """prints the worst e_gpu / bound per family seen by this run (the module docstring's observed lines are a copy of it)"""
    for fam in sorted(WORST):
        print(f"worst e_gpu / bound  {fam:24s} {WORST[fam]:.3f}")
