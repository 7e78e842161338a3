"""GPU: the glue kernels of the in-place residual dense block (csrc/dense.hip: tpgsr_leaky_relu_window, tpgsr_scaled_add,
tpgsr_dense_bwd_step) alone against float64, and the convolution kernels run IN PLACE (input and output windows of one buffer) on every
forward route the RRDB shapes take.

Error rule: the `arith` rule of tests/kernel_table.py -- e_gpu <= 4 * e_ref32 + 4 * 2^-24 with e = max |got - ref64| / max |ref64| and
e_ref32 the float32-CPU error of the same expression; nothing in a bound comes from the GPU result.  In-place LeakyReLU and the
derivative mask are one rounded product at most: compared bitwise with the float32 CPU expression.

Shapes: M = 15 (a scalar tail, no multiple of 4 rows per block) and M = 1030 (more than one block); windows (ld, coff, C) = (192, 64, 32),
(192, 160, 32), (24, 8, 4) on the 16-byte path and (7, 2, 3), misaligned, on the element path.  Every buffer is NaN outside its windows
and carries one NaN guard row behind M: both must come back untouched."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_table import DEV, F64, FLOOR, _gen, err  # noqa: E402

MS = (15, 1030)
WINDOWS = ((192, 64, 32), (192, 160, 32), (24, 8, 4), (7, 2, 3))
SLOPE = 0.2
NAN = float("nan")


def _buf(M, ld, coff, C, key, special=False):
    """[M + 1][ld] float32: N(0, 1) inside the window of the first M rows (special: with +0.0, -0.0 and sure negatives), NaN elsewhere"""
    b = torch.full((M + 1, ld), NAN)
    w = torch.randn(M, C, generator=_gen("dense", key, M, ld, coff, C))
    if special:
        flat = w.reshape(-1)
        flat[0::7] = 0.0
        flat[3::7] = -0.0
        flat[5::7] = -flat[5::7].abs() - 0.5
    b[:M, coff:coff + C] = w
    return b


def _untouched(got, M, coff, C, tag):
    """everything outside the window of the first M rows is still NaN"""
    mask = torch.ones_like(got, dtype=torch.bool)
    mask[:M, coff:coff + C] = False
    assert torch.isnan(got[mask]).all(), f"{tag}: a column outside the window or the guard row was written"
    assert not torch.isnan(got[:M, coff:coff + C]).any(), f"{tag}: NaN inside the window"


def _arith(tag, got, ref64, ref32):
    e_gpu, e32 = err(got, ref64), err(ref32, ref64)
    bound = 4 * e32 + FLOOR
    print(f"{tag}: e_gpu {e_gpu:.2e}  e_ref32 {e32:.2e}  bound {bound:.2e}")
    assert e_gpu <= bound, (tag, e_gpu, bound)


def _leaky32(x, v, slope=SLOPE):
    return torch.where(x > 0, v, v * torch.tensor(slope, dtype=v.dtype))


# ---- tpgsr_leaky_relu_window ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("win", WINDOWS)
def test_leaky_relu_window(M, win):
    from tpgsr_amd import kernels as K
    ld, coff, C = win
    b = _buf(M, ld, coff, C, "lrelu", special=True)
    d = b.to(DEV)
    K.leaky_relu_window(d, ld, coff, C, M, SLOPE)
    torch.cuda.synchronize()
    got = d.cpu()
    _untouched(got, M, coff, C, f"leaky_relu_window {win} M {M}")
    x = b[:M, coff:coff + C]
    assert torch.equal(got[:M, coff:coff + C], _leaky32(x, x))
    assert (x == 0).any() and (x < 0).any() and (x > 0).any()


# ---- tpgsr_scaled_add ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("win", WINDOWS)
@pytest.mark.parametrize("mode", ["separate", "no_b", "onto_a", "onto_b"])
def test_scaled_add(M, win, mode):
    """a in a window, b dense [M][C], out in a window of its own buffer (separate / no_b), or aliasing a or b window for window"""
    from tpgsr_amd import kernels as K
    ld, coff, C = win
    alpha = 0.2
    a = _buf(M, ld, coff, C, "sa_a")
    bb = _buf(M, C, 0, C, "sa_b")
    out = torch.full((M + 1, ld), NAN)
    da, db, do = a.to(DEV), bb.to(DEV), out.to(DEV)
    if mode == "separate":
        K.scaled_add(da, ld, coff, db, C, 0, alpha, do, ld, coff, M, C)
        res, (rl, rc) = do, (ld, coff)
    elif mode == "no_b":
        K.scaled_add(da, ld, coff, None, 0, 0, alpha, do, ld, coff, M, C)
        res, (rl, rc) = do, (ld, coff)
    elif mode == "onto_a":
        K.scaled_add(da, ld, coff, db, C, 0, alpha, da, ld, coff, M, C)
        res, (rl, rc) = da, (ld, coff)
    else:
        K.scaled_add(da, ld, coff, db, C, 0, alpha, db, C, 0, M, C)
        res, (rl, rc) = db, (C, 0)
    torch.cuda.synchronize()
    got = res.cpu()
    tag = f"scaled_add {mode} {win} M {M}"
    _untouched(got, M, rc, C, tag)
    if mode not in ("onto_a",):
        assert torch.equal(torch.nan_to_num(da.cpu(), nan=7.0), torch.nan_to_num(a, nan=7.0)), f"{tag}: a was written"
    if mode not in ("onto_b",):
        assert torch.equal(torch.nan_to_num(db.cpu(), nan=7.0), torch.nan_to_num(bb, nan=7.0)), f"{tag}: b was written"
    A, B = a[:M, coff:coff + C], bb[:M, :C]
    al32 = torch.tensor(alpha, dtype=torch.float32)
    if mode == "no_b":
        ref32, ref64 = al32 * A, al32.double() * A.double()
    else:
        ref32, ref64 = al32 * A + B, al32.double() * A.double() + B.double()
    _arith(tag, got[:M, rc:rc + C], ref64, ref32)


# ---- tpgsr_dense_bwd_step ------------------------------------------------------------------------------------------------------------
#            ld, c_acc, mask_coff, mask_c, with T
STEP_CASES = [(192, 64, 32, 32, True),        # accumulate + mask (16-byte path)
              (24, 8, 0, 0, True),            # accumulate only (mask_c = 0)
              (192, 192, 160, 32, False),     # the first call of a block: mask only, T = NULL
              (7, 5, 2, 3, True),             # misaligned: the element path
              (7, 5, 2, 3, False)]


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("case", STEP_CASES, ids=lambda c: "ld%d-acc%d-mask%d+%d-%s" % (c[0], c[1], c[2], c[3], "T" if c[4] else "noT"))
def test_dense_bwd_step(M, case):
    from tpgsr_amd import kernels as K
    ld, c_acc, mcoff, mc, with_t = case
    G = _buf(M, ld, 0, c_acc, "step_g")
    T = _buf(M, c_acc, 0, c_acc, "step_t")[:M].contiguous()
    D = _buf(M, ld, mcoff, max(mc, 1), "step_d", special=True)      # NaN outside the mask window: reading it there would poison G
    if mc == 0:
        D[:] = NAN
    dG, dT, dD = G.to(DEV), T.to(DEV), D.to(DEV)
    K.dense_bwd_step(dG, ld, dT if with_t else None, c_acc, dD, mcoff, mc, SLOPE, M)
    torch.cuda.synchronize()
    got = dG.cpu()
    tag = f"dense_bwd_step {case} M {M}"
    _untouched(got, M, 0, c_acc, tag)
    assert torch.equal(torch.nan_to_num(dD.cpu(), nan=7.0), torch.nan_to_num(D, nan=7.0)) and torch.equal(dT.cpu(), T)
    g = G[:M, :c_acc]
    s32 = g + T if with_t else g.clone()
    s64 = g.double() + T.double() if with_t else g.double()
    if mc:
        d = D[:M, mcoff:mcoff + mc]
        s32[:, mcoff:mcoff + mc] = _leaky32(d, s32[:, mcoff:mcoff + mc])
        w64 = s64[:, mcoff:mcoff + mc]
        s64[:, mcoff:mcoff + mc] = torch.where(d > 0, w64, w64 * torch.tensor(SLOPE, dtype=torch.float32).double())
        # the derivative at +0.0 and at -0.0 is `slope`
        zero = torch.zeros(M, c_acc, dtype=torch.bool)
        zero[:, mcoff:mcoff + mc] = d == 0
        assert zero.any() and (torch.signbit(d) & (d == 0)).any() and (~torch.signbit(d) & (d == 0)).any()
        pre = (g + T) if with_t else g
        assert torch.equal(got[:M, :c_acc][zero], (pre * torch.tensor(SLOPE))[zero])
    if with_t:
        _arith(tag, got[:M, :c_acc], s64, s32)
    else:
        assert torch.equal(got[:M, :c_acc], s32), tag      # the mask alone: exact
        if mc < c_acc:      # columns of the prefix outside the mask window are not even visited
            keep = torch.ones(c_acc, dtype=torch.bool)
            keep[mcoff:mcoff + mc] = False
            assert torch.equal(got[:M, :c_acc][:, keep], g[:, keep])


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("ld,c_acc", [(192, 64), (7, 3)])
@pytest.mark.parametrize("with_skip", [True, False])
def test_dense_bwd_step_final(M, ld, c_acc, with_skip):
    """the last pass: dx = (G[:, :c_acc] + T) + skip, G itself unchanged"""
    from tpgsr_amd import kernels as K
    G = _buf(M, ld, 0, c_acc, "fin_g")
    T = _buf(M, c_acc, 0, c_acc, "fin_t")[:M].contiguous()
    S = _buf(M, c_acc, 0, c_acc, "fin_s")[:M].contiguous()
    dx = torch.full((M + 1, c_acc), NAN)
    dG, dT, dS, ddx = G.to(DEV), T.to(DEV), S.to(DEV), dx.to(DEV)
    K.dense_bwd_step(dG, ld, dT, c_acc, None, 0, 0, SLOPE, M, skip=dS if with_skip else None, dx=ddx)
    torch.cuda.synchronize()
    got = ddx.cpu()
    tag = f"dense_bwd_step final ld {ld} c_acc {c_acc} M {M} skip {with_skip}"
    _untouched(got, M, 0, c_acc, tag)
    assert torch.equal(torch.nan_to_num(dG.cpu(), nan=7.0), torch.nan_to_num(G, nan=7.0)), f"{tag}: G was written"
    g = G[:M, :c_acc]
    r32, r64 = g + T, g.double() + T.double()
    if with_skip:
        r32, r64 = r32 + S, r64 + S.double()
    _arith(tag, got[:M], r64, r32)


def test_bad_arguments_are_refused():
    from tpgsr_amd import kernels as K
    b = torch.zeros(4, 8, device=DEV)
    t = torch.zeros(4, 4, device=DEV)
    with pytest.raises(Exception, match="tpgsr_leaky_relu_window"):
        K.leaky_relu_window(b, 8, 6, 4, 4, SLOPE)                     # the window leaves the row
    with pytest.raises(Exception, match="tpgsr_scaled_add"):
        K.scaled_add(b, 8, 0, None, 0, 0, 0.2, b, 8, 6, 4, 4)
    with pytest.raises(Exception, match="tpgsr_dense_bwd_step"):
        K.dense_bwd_step(b, 8, t, 4, b, 2, 4, SLOPE, 4)               # the mask window leaves [0, c_acc)
    with pytest.raises(Exception, match="tpgsr_dense_bwd_step"):
        K.dense_bwd_step(b, 8, None, 4, b, 0, 0, SLOPE, 4)            # nothing to do
    torch.cuda.synchronize()


# ---- the convolution kernels in place ------------------------------------------------------------------------------------------------
# (Cin, Cout, ld): the four growing convolutions of a block write the window behind their input prefix; conv5 (192 -> 64) writes a dense
# tensor in the block -- here it gets a 256-column buffer so that its route is run with in == out as well
RRDB_CONVS = ((64, 32, 192), (96, 32, 192), (128, 32, 192), (160, 32, 192), (192, 64, 256))


@pytest.mark.parametrize("N", [1, 48], ids=["M1024", "M49152"])
@pytest.mark.parametrize("prec", ["x3", "x2"])
def test_convolution_in_place_on_every_route(N, prec):
    """conv_fwd with in == out and disjoint channel windows against the same launch into a separate buffer: the window bit-identical, the
    input columns unchanged; every RRDB shape, whatever forward route it takes (printed)"""
    from tpgsr_amd import functional as Fh
    from tpgsr_amd import kernels as K
    H, W = 16, 64
    M = N * H * W
    seen = set()
    with K.policy(prec):
        for Cin, Cout, ld in RRDB_CONVS:
            g = _gen("inplace", Cin, Cout)
            w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (3 * Cin ** 0.5)).to(DEV)
            bias = (0.1 * torch.randn(Cout, generator=g)).to(DEV)
            wt_f, *_ = Fh._pack(w, False, 1.0)
            geom = K.ConvGeom(N, H, W, Cin, Cout, 3, 3, 1, 1)
            D = torch.full((M + 1, ld), NAN, device=DEV)
            D[:M, :Cin] = torch.randn(M, Cin, generator=_gen("inplace_x", Cin, N)).to(DEV)
            D[:M, Cin:Cin + Cout] = 0.0       # (the separate launch reads nothing there either; NaN behind the window stays)
            O2 = torch.full((M + 1, ld), NAN, device=DEV)
            args = K.make_conv_args(geom, D, wt_f, D, bias=bias, in_ld=ld, out_ld=ld, out_coff=Cin)
            name, r = K.conv_route(args)
            seen.add((name, r.ld, r.nbw, r.lcap, r.splits))      # (shapes that share a route are run all the same: a launch each)
            before = D.clone()
            K.conv_fwd(K.make_conv_args(geom, D, wt_f, O2, bias=bias, in_ld=ld, out_ld=ld, out_coff=Cin))
            K.conv_fwd(args)
            torch.cuda.synchronize()
            print(f"{prec} M {M} {Cin} -> {Cout} (ld {ld}): {name}")
            assert name != "none"
            assert torch.equal(D[:M, Cin:Cin + Cout], O2[:M, Cin:Cin + Cout]), (name, Cin)
            assert not torch.isnan(D[:M, Cin:Cin + Cout]).any()
            assert torch.equal(D[:M, :Cin], before[:M, :Cin]), f"{name}: the input columns changed"
            assert torch.isnan(D[:M, Cin + Cout:]).all() and torch.isnan(D[M]).all() and torch.isnan(O2[M]).all()
            assert torch.isnan(O2[:M, :Cin]).all() and torch.isnan(O2[:M, Cin + Cout:]).all()
    assert seen
