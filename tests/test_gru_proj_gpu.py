"""GPU: the GruBlock forward as ONE launch (csrc/gru_proj.hip: the composed input projection on the matrix cores into LDS + the
bidirectional scan) against the two launches it replaces (tpgsr_conv_fwd into a [P][192] map + tpgsr_bigru_fwd) and against nn.GRU's gate
equations in fp64 -- every loader the SR network uses (plain, BatchNorm affine, residual add, affine + concatenated text strip), both scan
axes of the 16 x 64 map, two- and three-term arithmetic, training (gates stored) and inference.  Reference: GruBlock, model/tsrn.py:491-508;
RecurrentResidualBlockTL, model/tsrn.py:411-426."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _case(N, H, W, Cin, loader, seed, dev=None):
    dev = DEV if dev is None else dev
    g = torch.Generator().manual_seed(seed)
    P = N * H * W
    t = dict(x=torch.randn(P, 64, generator=g), wc=torch.randn(Cin, 192, generator=g) / Cin ** 0.5, bc=torch.randn(192, generator=g) * 0.1,
             whh=torch.randn(2, 96, 32, generator=g) / 32 ** 0.5, bhh=torch.randn(2, 96, generator=g) * 0.1)
    kw = {}
    if loader in ("affine", "affine+strip"):
        t["scale"], t["shift"] = torch.rand(Cin, generator=g) + 0.5, torch.randn(Cin, generator=g)
        if loader == "affine+strip":
            t["scale"][64:], t["shift"][64:] = 1.0, 0.0                 # (engine.BNLayer pads its scale / shift with the identity)
            t["strip"] = torch.randn(N * W, 32, generator=g)
    if loader == "residual":
        t["x2"] = torch.randn(P, 64, generator=g)
    t = {k: v.to(dev).contiguous() for k, v in t.items()}
    if "scale" in t:
        kw.update(in_scale=t["scale"], in_shift=t["shift"])
    if "strip" in t:
        kw.update(in_b=t["strip"], cin_a=64)
    if "x2" in t:
        kw.update(in2=t["x2"])
    return t, kw


def _reference_fp64(t, N, H, W, Cin, axis, planes=False, bf16=False):
    """nn.GRU's equations (gate order r, z, n) on the fp64 projection of the loader's output; planes: also the stored gate planes
    [P][256] = per direction (r, z, n, W_hn h + b_hn); bf16: the loader's output and Wc each rounded to bf16 first (round to nearest even:
    the operands of one-term arithmetic), everything else in fp64 as before"""
    x = t["x"].double().cpu().view(N, H, W, 64)
    if "scale" in t:
        x = x * t["scale"][:64].double().cpu() + t["shift"][:64].double().cpu()
    if "x2" in t:
        x = x + t["x2"].double().cpu().view(N, H, W, 64)
    if "strip" in t:
        x = torch.cat([x, t["strip"].double().cpu().view(N, 1, W, 32).expand(N, H, W, 32)], -1)
    wc = t["wc"].double().cpu()
    if bf16:
        x, wc = x.to(torch.bfloat16).double(), wc.to(torch.bfloat16).double()
    gi = x @ wc + t["bc"].double().cpu()                                 # [N][H][W][192]
    if axis == 1:
        gi = gi.transpose(1, 2)                                          # sequences along H: [N][W][H][192]
    S, T = gi.shape[0] * gi.shape[1], gi.shape[2]
    gi = gi.reshape(S, T, 192)
    whh, bhh = t["whh"].double().cpu(), t["bhh"].double().cpu()
    out = torch.zeros(S, T, 64, dtype=torch.float64)
    gt = torch.zeros(S, T, 256, dtype=torch.float64)
    for d in range(2):
        h = torch.zeros(S, 32, dtype=torch.float64)
        for step in (range(T) if d == 0 else range(T - 1, -1, -1)):
            gh = h @ whh[d].T + bhh[d]
            g_ = gi[:, step, 96 * d:96 * d + 96]
            r = torch.sigmoid(g_[:, :32] + gh[:, :32])
            z = torch.sigmoid(g_[:, 32:64] + gh[:, 32:64])
            n = torch.tanh(g_[:, 64:] + r * gh[:, 64:])
            h = (1 - z) * n + z * h
            out[:, step, 32 * d:32 * d + 32] = h
            gt[:, step, 128 * d:128 * d + 128] = torch.cat([r, z, n, gh[:, 64:]], 1)
    out, gt = out.view(-1, (W if axis == 1 else H), T, 64), gt.view(-1, (W if axis == 1 else H), T, 256)
    if axis == 1:
        out, gt = out.transpose(1, 2), gt.transpose(1, 2)
    if planes:
        return out.reshape(N * H * W, 64), gt.reshape(N * H * W, 256)
    return out.reshape(N * H * W, 64)


@pytest.mark.parametrize("terms", [2, 3])
@pytest.mark.parametrize("axis,loader", [(0, "residual"), (0, "plain"), (1, "affine+strip"), (1, "affine"), (1, "plain"), (0, "affine")])
def test_one_launch_gru_block_forward(axis, loader, terms):
    from tpgsr_amd import kernels as K
    N, H, W = 3, 16, 64
    Cin = 96 if loader == "affine+strip" else 64
    t, kw = _case(N, H, W, Cin, loader, seed=17 * axis + terms)
    P = N * H * W
    geom = K.ConvGeom(N, H, W, Cin, 192)
    with K.conv_terms(terms):
        K.make_bf_twin(t["wc"], 0)
        # two launches
        gi, h0, gt0 = torch.empty(P, 192, device=DEV), torch.empty(P, 64, device=DEV), torch.empty(P, 256, device=DEV)
        K.conv_fwd(K.make_conv_args(geom, t["x"], t["wc"], gi, bias=t["bc"], **kw))
        K.bigru_fwd(gi, t["whh"], t["bhh"], N, H, W, axis, h0, gt0)
        # one launch, training and inference
        h1, gt1, h2 = torch.full((P, 64), float("nan"), device=DEV), torch.full((P, 256), float("nan"), device=DEV), torch.full((P, 64), float("nan"), device=DEV)
        pa = K.make_bigru_proj_args(K.make_conv_args(geom, t["x"], t["wc"], None, bias=t["bc"], **kw), t["whh"], t["bhh"], axis, h1, gt1)
        assert K.bigru_proj_supported(pa)
        K.bigru_proj_fwd(pa)
        K.bigru_proj_fwd(K.make_bigru_proj_args(K.make_conv_args(geom, t["x"], t["wc"], None, bias=t["bc"], **kw), t["whh"], t["bhh"], axis, h2, None))
        h3 = torch.empty_like(h1)
        K.bigru_proj_fwd(K.make_bigru_proj_args(K.make_conv_args(geom, t["x"], t["wc"], None, bias=t["bc"], **kw), t["whh"], t["bhh"], axis, h3, None))
    torch.cuda.synchronize()
    ref = _reference_fp64(t, N, H, W, Cin, axis)
    e_two, e_one = (h0.double().cpu() - ref).abs().max().item(), (h1.double().cpu() - ref).abs().max().item()
    print(f"axis {axis} {loader} x{terms}: max |h - fp64| two launches {e_two:.2e}, one launch {e_one:.2e}; one vs two {float((h1 - h0).abs().max()):.2e}")
    tol = 8e-5 if terms == 2 else 3e-6            # (two-term split: ~16 significand bits per operand, the scan feeds it back 64 times)
    assert e_one < tol and e_one < 2 * e_two + 1e-6
    assert (h1 - h0).abs().max() < tol and (gt1 - gt0).abs().max() < 2 * tol
    assert torch.equal(h1, h2) and torch.equal(h2, h3)          # inference variant == training variant, bitwise repeatable


def test_shapes_the_fused_kernel_does_not_take_fall_back_loudly():
    from tpgsr_amd import kernels as K
    from tpgsr_amd._lib import TpgsrKernelError
    N, H, W = 2, 8, 32                                           # scan lengths 8 / 32: not this kernel's
    t, kw = _case(N, H, W, 64, "plain", 1)
    geom = K.ConvGeom(N, H, W, 64, 192)
    with K.conv_terms(2):
        K.make_bf_twin(t["wc"], 0)
        h = torch.empty(N * H * W, 64, device=DEV)
        pa = K.make_bigru_proj_args(K.make_conv_args(geom, t["x"], t["wc"], None, bias=t["bc"]), t["whh"], t["bhh"], 0, h, None)
        assert not K.bigru_proj_supported(pa)
        with pytest.raises(TpgsrKernelError, match="not the fused kernel"):
            K.bigru_proj_fwd(pa)
    with K.conv_terms(0):                                        # fp32 matrix cores: no split planes
        pa = K.make_bigru_proj_args(K.make_conv_args(K.ConvGeom(3, 16, 64, 64, 192), t["x"], t["wc"], None, bias=t["bc"]), t["whh"], t["bhh"], 0, h, None)
        assert not K.bigru_proj_supported(pa)


@pytest.mark.parametrize("terms", [2, 3])
@pytest.mark.parametrize("axis,loader", [(1, "affine"), (1, "affine+strip"), (0, "residual")])
def test_full_batch_is_bitwise_repeatable_and_per_sequence(axis, loader, terms):
    """bs 48 (3072 / 768 workgroups, several per CU): ten launches give the same bits, and a batch permutation permutes the result --
    what tests/test_tsrn_gpu.py::test_full_size_properties_bs48 and the schedule tests need from every forward kernel.  (A first
    four-wave form of the kernel -- column tiles 3 w .. 3 w + 2 per wave, fully unrolled -- passed every small test and failed exactly this
    under three-term arithmetic, for a reason its ISA does not show: both forms wait for their LDS stores in front of the barrier.)"""
    from tpgsr_amd import kernels as K
    N, H, W = 48, 16, 64
    Cin = 96 if loader == "affine+strip" else 64
    t, kw = _case(N, H, W, Cin, loader, seed=5)
    P = N * H * W
    geom = K.ConvGeom(N, H, W, Cin, 192)
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(2)).to(DEV)

    def permuted(v, rows_per_image):
        return v.view(N, rows_per_image, -1)[perm].reshape(v.shape).contiguous()

    with K.conv_terms(terms):
        K.make_bf_twin(t["wc"], 0)
        outs = []
        for rep in range(10):
            h, gt = torch.full((P, 64), float("nan"), device=DEV), torch.full((P, 256), float("nan"), device=DEV)
            K.bigru_proj_fwd(K.make_bigru_proj_args(K.make_conv_args(geom, t["x"], t["wc"], None, bias=t["bc"], **kw), t["whh"], t["bhh"], axis, h, gt))
            outs.append((h, gt))
        tp = dict(t)
        tp["x"] = permuted(t["x"], H * W)
        kwp = dict(kw)
        if "x2" in t:
            kwp["in2"] = permuted(t["x2"], H * W)
        if "strip" in t:
            kwp["in_b"] = permuted(t["strip"], W)
        hp = torch.empty(P, 64, device=DEV)
        K.bigru_proj_fwd(K.make_bigru_proj_args(K.make_conv_args(geom, tp["x"], t["wc"], None, bias=t["bc"], **kwp), t["whh"], t["bhh"], axis, hp, None))
    torch.cuda.synchronize()
    for h, gt in outs[1:]:
        assert torch.equal(h, outs[0][0]) and torch.equal(gt, outs[0][1])
    assert torch.equal(hp, permuted(outs[0][0], H * W))


# ---- the whole supported matrix against fp64 ------------------------------------------------------------------------------------------
# the smallest maps that reach every (NRT, NKS) of bigru_proj_fwd_kernel<LD, TT, NRT, NKS, TRAIN>: (N, H, W, axis)
MATRIX_MAPS = [(1, 1, 64, 0), (2, 3, 64, 0),         # T = 64 along W; H > 1: the strip's (n, w) row is shared by three sequences
               (1, 64, 3, 1),                        # T = 64 along H
               (1, 16, 4, 1), (1, 16, 12, 1),        # T = 16 along H: four sequences to a workgroup, one and three workgroups
               (1, 4, 16, 0), (2, 6, 16, 0)]         # T = 16 along W
MATRIX_LOADERS = ["plain", "affine", "residual", "affine+strip"]
PLANES = ("r", "z", "n", "W_hn h + b_hn")
_MATRIX_REF = {}
WORST = {}          # (terms, "h" or "planes") -> worst e / bound seen by test_fused_forward_matrix_vs_fp64


def _plane(gt, k):
    """plane k of both directions out of [P][256]"""
    return torch.cat([gt[:, 32 * k:32 * k + 32], gt[:, 128 + 32 * k:128 + 32 * k + 32]], 1)


def matrix_reference(N, H, W, axis, loader):
    """(fp64 h, fp64 gate planes, e_model of h, e_model per plane), once per case: e_model = max |.| between the fp64 recurrence on
    bf16-rounded operands and the unrounded one -- what one-term arithmetic costs, from the reference alone"""
    key = (N, H, W, axis, loader)
    if key not in _MATRIX_REF:
        Cin = 96 if loader == "affine+strip" else 64
        t, _ = _case(N, H, W, Cin, loader, seed=1000 * H + W + 7 * axis + len(loader), dev="cpu")
        h, gt = _reference_fp64(t, N, H, W, Cin, axis, planes=True)
        hm, gm = _reference_fp64(t, N, H, W, Cin, axis, planes=True, bf16=True)
        _MATRIX_REF[key] = (h, gt, (hm - h).abs().max().item(), [(_plane(gm, k) - _plane(gt, k)).abs().max().item() for k in range(4)])
    return _MATRIX_REF[key]


@pytest.mark.parametrize("loader", MATRIX_LOADERS)
@pytest.mark.parametrize("N,H,W,axis", MATRIX_MAPS)
def test_fused_forward_matrix_vs_fp64(N, H, W, axis, loader):
    """every loader x terms {1, 2, 3} x gates stored or not, on every map of MATRIX_MAPS: h and the four stored planes against the fp64
    recurrence.  Bounds (absolute): terms 3 / 2 -- this file's own 3e-6 / 8e-5 for h and twice that for the planes, the numbers
    test_one_launch_gru_block_forward asserts against the two-launch path; terms 1 -- 4 e_model + the terms-3 bound (e_model: see
    matrix_reference; the factor 4 is the suite's margin and absorbs a bf16 rounding flipped by the loader's fp32 multiply-add)"""
    from tpgsr_amd import kernels as K
    Cin = 96 if loader == "affine+strip" else 64
    t, kw = _case(N, H, W, Cin, loader, seed=1000 * H + W + 7 * axis + len(loader))
    P = N * H * W
    geom = K.ConvGeom(N, H, W, Cin, 192)
    ref_h, ref_gt, em_h, em_gt = matrix_reference(N, H, W, axis, loader)
    bad = []
    for terms in (3, 2, 1):
        tol = {3: 3e-6, 2: 8e-5, 1: 3e-6}[terms]
        with K.conv_terms(terms):
            K.make_bf_twin(t["wc"], 0)
            outs = []
            for train in (True, False):
                h = torch.full((P, 64), float("nan"), device=DEV)
                gt = torch.full((P, 256), float("nan"), device=DEV) if train else None
                pa = K.make_bigru_proj_args(K.make_conv_args(geom, t["x"], t["wc"], None, bias=t["bc"], **kw), t["whh"], t["bhh"], axis, h, gt)
                assert K.bigru_proj_supported(pa)
                K.bigru_proj_fwd(pa)
                outs.append((h, gt))
        torch.cuda.synchronize()
        for (h, gt), train in zip(outs, (True, False)):
            what = f"{N}x{H}x{W} axis {axis} {loader} x{terms} {'train' if train else 'eval'}"
            bound = 4 * em_h + tol if terms == 1 else tol
            e = (h.double().cpu() - ref_h).abs().max().item()
            WORST[terms, "h"] = max(WORST.get((terms, "h"), 0.0), e / bound)
            print(f"{what}: max |h - fp64| {e:.2e}  bound {bound:.2e}")
            if not e <= bound:
                bad.append(f"{what} h: {e:.3e} > {bound:.3e}")
            if train:
                for k, name in enumerate(PLANES):
                    bound = 4 * em_gt[k] + 2 * tol if terms == 1 else 2 * tol
                    e = (_plane(gt.double().cpu(), k) - _plane(ref_gt, k)).abs().max().item()
                    WORST[terms, "planes"] = max(WORST.get((terms, "planes"), 0.0), e / bound)
                    print(f"{what}: max |{name} - fp64| {e:.2e}  bound {bound:.2e}")
                    if not e <= bound:
                        bad.append(f"{what} {name}: {e:.3e} > {bound:.3e}")
    assert not bad, "; ".join(bad)


def test_sixteen_step_scans_need_a_multiple_of_four_sequences():
    """T = 16 with three sequences (1 x 16 x 3 along H): four sequences go to a workgroup, so this block is not the fused kernel's"""
    from tpgsr_amd import kernels as K
    from tpgsr_amd._lib import TpgsrKernelError
    N, H, W = 1, 16, 3
    t, kw = _case(N, H, W, 64, "plain", 3)
    with K.conv_terms(2):
        K.make_bf_twin(t["wc"], 0)
        h = torch.empty(N * H * W, 64, device=DEV)
        pa = K.make_bigru_proj_args(K.make_conv_args(K.ConvGeom(N, H, W, 64, 192), t["x"], t["wc"], None, bias=t["bc"]), t["whh"], t["bhh"], 1, h, None)
        assert not K.bigru_proj_supported(pa)
        with pytest.raises(TpgsrKernelError, match="not the fused kernel"):
            K.bigru_proj_fwd(pa)


def test_zz_report():
    """observed on an MI355X, worst e / bound of the matrix: h 0.24 / 0.35 / 0.25 under terms 3 / 2 / 1, gate planes 0.16 / 0.22 / 0.25"""
    for terms, what in sorted(WORST, reverse=True):
        print(f"one-launch forward vs fp64, terms {terms}, {what}: worst e / bound {WORST[terms, what]:.2f}")
