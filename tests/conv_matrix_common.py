"""Every instantiated convolution kernel variant, route asserted: the case table and the references shared by
tests/test_conv_matrix_cpu.py and tests/test_conv_matrix_gpu.py (a harness, not a conftest).

tpgsr_conv_fwd / tpgsr_conv_wgrad / tpgsr_conv_wgrad_batch run one of eleven kernels, each a template over a loader variant `ld`
(1 affine, 2 activation, 4 residual add, 8 un-PixelShuffle gather, 16 concatenated strip, 32 scaled residual) and a term count T; the
launchers' switch tables instantiate the (kernel, ld, T, shape class) combinations of KERNELS below.  CASES holds one case per
combination, the epilogue / operand-window classes of EPI rotating over them so that every class a kernel supports appears for every T,
plus the (kernel, ld, epilogue) combinations the engines' recorded launches use (RECORDED).  A case names the smallest geometry the route
sends to its kernel under the library's default switches (setters only where a threshold cannot be met on a small map: KNOBS), with the
edges the kernel's indexing depends on: ragged M, ragged Cout (37, 40, 72, 100, 500), tiles spanning rows and images, N = 1.

`block(case, ptrs)` builds the argument block from the case alone (fake aligned pointers on the CPU, device pointers on the GPU), so the
route the CPU test pins is the route of the block the GPU test launches.

References (CPU, stock PyTorch, nothing from the kernels):
  truth    the loader written out in float64 -- act(in * scale + shift) + in2 [* in2_scale], un-PixelShuffle, channel concat with the
           strip broadcast over H, zero dilation, zero padding AFTER the loader -- then im2col (F.unfold) and a float64 matmul, then the
           epilogue: bias, activation, pixel shuffle, sum / sum of squares of (out - bias) per 64 (192) pixel row block, or the
           BatchNorm-backward sums  sum dz, sum dz * xhat,  dz = da * act'(y * scale + shift)  and out = dz under bnb_store_dz.
  model    the same in float64 on operands split as DESIGN 4.1 states: x1 = bf16(x), x2 = bf16(x - x1), x3 = bf16(x - x1 - x2); kept
           products T = 1: a1 b1; T = 2: a1 b1 + a1 b2 + a2 b1; T = 3: the six with i + j <= 4 (T = 0, the fp32 kernels: the unsplit
           product).  The loader's output is rounded to fp32 before the split (the kernels split after the loader); for weight gradients
           both A and dy are split.
  ref32    the truth's computation in float32 on the CPU.

Bounds (`bounds(case)`; nothing in them comes from a GPU result), e = max |got - ref| / max |ref| (`err`):
  against the truth   engine_layer_common.limits(policy): f32 and x3 5e-6 for values and data gradients, 1e-5 for weight and bias
                      gradients; x2 2e-5; bf16 2e-2.  The limits are relative to the largest element of a LINEAR result.  Behind an
                      output activation (ReLU, tanh: Lipschitz constant 1) the accumulator's absolute error passes through unchanged
                      while the scale shrinks (tanh: to 1), so the limit for `out` is multiplied by max |out before the activation| /
                      max |out| of the float64 truth (>= 1; 1 without an activation).  Statistics rows: 4 x the value limit for sum / sum of squares (2e-5 at x3, what
                      the family tests assert), 8 x for the BatchNorm-backward sums (tests/test_bnb_fuse_gpu.py).
  against the model   for every T the x3 limits (5e-6 / 1e-5) + 4 d_loader + 4 d_ulp.
                      d_loader = err(model with the loader in float32 on the CPU, model with the loader in float64): a one-ulp
                      difference in the loader's fp32 result flips a bf16 rounding of the element.  Zero for loaders without arithmetic.
                      d_ulp = the larger err of the model with the float64 loader's fp32 result moved one ulp up / one ulp down: the CPU's
                      float32 loader and the GPU's (fused multiply-adds, its own mish) differ from the float64 one in DIFFERENT
                      elements, and whether an element sits on a bf16 rounding boundary is a lottery of a few elements per case -- the two
                      shifted evaluations flip every element within one ulp of a boundary, on either side, which is what a loader one ulp
                      off can flip at most.  Zero where d_loader is zero by construction.  At T = 1 one flip is 2^-8 of a product, which is
                      why these terms and not a constant: a dropped correction product or a wrong channel is orders above them.
                      Statistics rows: the `arith` rule of tests/kernel_table.py, e <= 4 e_ref32 + 4 * 2^-24 (kernel_table.bound_of) plus
                      the two loader terms of that key, capped by what the family tests assert: 2e-5 for sum / sum of squares, 8 x the
                      value limit for the BatchNorm-backward sums.
Pre-fills: outputs are NaN before the launch; columns outside Cout / the out_coff window, one guard row behind M, one guard row behind
the statistics and one guard slab behind the weight-gradient splits must keep it.
ReLU in a loader or in bnb_act: `margin_of(case, operands)` -- min |z| over the case exceeds 1e-4, the seed scanned as POOL_SEEDS is (cases too large for
any seed to keep the margin use mish in the loader, and push the BatchNorm input away from the kink by construction)."""
import ctypes as C
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_functional_ops_gpu import CONV_LIMITS, F64, FLOOR, POOL_SEEDS, _gen, err  # noqa: E402,F401
from kernel_table import bound_of  # noqa: E402  (the `arith` rule: 4 e_ref32 + FLOOR, capped)
from engine_layer_common import limits  # noqa: E402

DEV = "cuda"
F32 = torch.float32
POLICY = {0: "f32", 1: "bf16", 2: "x2", 3: "x3"}
RELU_MARGIN = 1e-4
SIZE_LIMIT = 16 << 20
PTR = 0x10000000
MODEL_LIMITS = CONV_LIMITS["x3"]
STAT_CAP = 2e-5                      # sum / sum of squares against the model (test_conv_xbf_gpu / test_conv_panel_gpu)
FWD_STATS = ("sum", "sumsq", "sdz", "sdzx")

# switches a case may set: name -> (setter, default)
KNOBS = {"panel_min_m": ("tpgsr_panel_set_min_m", 32768), "panel_k192": ("tpgsr_panel_set_k192", 0),
         "colmajor": ("tpgsr_halo_set_colmajor_min_bytes", 3 << 20), "halo3": ("tpgsr_halo3_set_enabled", 1),
         "splitk": ("tpgsr_splitk_set_enabled", 1), "wgrad3": ("tpgsr_wgrad3_set_enabled", 1)}

ALL9 = (0, 1, 2, 3, 4, 5, 7, 8, 17)
WG8 = (0, 1, 2, 3, 4, 5, 7, 17)
HALO7 = (0, 1, 2, 3, 4, 5, 7)

# ---- epilogue / operand-window classes ---------------------------------------------------------------------------------------------
#  bias relu tanh ps(out_ps) bn(bn_partial) rt3(bn_row_tiles = 3) bnb0 / bnb1 / bnb2 (BatchNorm-backward sums, act none / relu / mish)
#  dz(bnb_store_dz) dzonly(bnb_store_dz without sums, mish) outwin(out_ld / out_coff) wtwin(wt_ld / wt_coff) inwin(in_ld / in_coff)
#  stride(stride_w = 2) dil(in_dil_w = 2);  weight gradients: db(dbpart) dywin(dy_ld / dy_coff) dyps(dy_ps) z(explicit zsplits)
F32_EPI = [(), ("bias",), ("bias", "relu"), ("bias", "tanh"), ("bias", "ps"), ("bias", "bn"), ("bn",), ("outwin", "bias"), ("wtwin", "bias"),
           ("inwin",), ("wtwin", "stride"), ("bn", "dil"), ("stride", "bias"), ("dil",)]
XBF_EPI = [(), ("bias",), ("bias", "relu"), ("bias", "tanh"), ("bias", "ps"), ("bias", "bn"), ("bn",), ("bnb0",), ("bnb1",), ("bnb2",),
           ("bnb2", "dz"), ("dzonly",), ("outwin", "bias"), ("wtwin", "bias"), ("inwin",)]
TILE_EPI = XBF_EPI + [("bnb1", "wtwin", "stride"), ("bn", "dil"), ("stride", "bias"), ("dil",), ("bnb0", "wtwin")]
HALO3_EPI = XBF_EPI + [("bias", "bn", "rt3"), ("bnb1", "rt3"), ("bnb2", "rt3"), ("bnb0", "rt3", "dz")]
WSTAT_EPI = [(), ("bias",), ("bias", "bn"), ("outwin", "bias"), ("inwin",), ("bn",)]
WG_EPI = [(), ("db",), ("db", "dywin"), ("db", "dywin", "inwin"), ("db", "z"), ("z",), ("dil",), ("stride", "db")]
WG_PS_EPI = [("dyps",), ("db", "dyps", "z"), ("dyps", "inwin"), ("db", "dyps")]
WG3_EPI = [("db", "z"), ("z",), ("db", "dywin"), (), ("db", "inwin")]
WGH_EPI = [("z",), ("db", "z"), ("db", "z", "inwin"), ("db", "z", "dywin"), ("db", "z", "dyps")]
BATCH_EPI = [("db",), ("db", "dywin"), ("db", "dywin", "inwin"), ()]

# ---- the matrix: (op, kernel) -> loader variants, terms, {shape class: (knobs, geometries (N, H, W, Cin, Cout, KH, KW, ph, pw))}, epilogues
# (f32_scalar's loader is a run-time branch: its cases are SCALAR_FWD / SCALAR_WG below)
G33 = [(1, 4, 16, 16, 64, 3, 3, 1, 1), (3, 5, 13, 16, 40, 3, 3, 1, 1), (2, 3, 7, 32, 37, 1, 1, 0, 0), (2, 6, 9, 16, 72, 2, 2, 0, 0)]
GSK = [(1, 4, 16, 16, 64, 3, 3, 1, 1), (3, 5, 13, 16, 40, 3, 3, 1, 1), (2, 3, 7, 64, 37, 1, 1, 0, 0), (2, 6, 9, 16, 72, 2, 2, 0, 0)]
GHALO = [(1, 4, 16, 32, 64, 3, 3, 1, 1), (3, 5, 13, 32, 40, 3, 3, 1, 1), (2, 3, 9, 32, 72, 1, 3, 0, 1), (1, 4, 16, 64, 100, 2, 2, 0, 0)]
GHCOL = [(1, 4, 16, 32, 128, 3, 3, 1, 1), (3, 5, 13, 32, 128, 3, 3, 1, 1)]
GH3 = [(6, 16, 48, 32, 512, 3, 3, 1, 1), (6, 16, 48, 32, 512, 3, 3, 1, 1), (6, 16, 48, 32, 512, 3, 3, 1, 1), (7, 11, 60, 32, 500, 3, 3, 1, 1)]
GH3G = [(6, 16, 48, 32, 512, 1, 3, 0, 1), (6, 16, 48, 32, 512, 1, 3, 0, 1), (6, 16, 48, 32, 512, 1, 3, 0, 1), (7, 11, 60, 32, 500, 1, 3, 0, 1)]
GPANEL = lambda ci, co: [(1, 8, 16, ci, co[0]), (3, 5, 9, ci, co[1]), (2, 7, 13, ci, co[2])]
SMALL_PANEL = {"panel_min_m": 64}
KERNELS = {
    ("fwd", "f32_tile"): (ALL9, (0,), {"": ({}, G33)}, F32_EPI),
    ("fwd", "f32_wstat"): ((0,), (0,), {"": ({}, [(1, 2, 64, 64, 64, 3, 3, 1, 1), (2, 3, 64, 64, 64, 3, 3, 1, 1)])}, WSTAT_EPI),
    ("fwd", "xbf_tile"): (ALL9, (1, 2, 3), {"": ({}, G33)}, TILE_EPI),
    ("fwd", "xbf_splitk"): (ALL9, (1, 2, 3), {"": ({}, GSK)}, TILE_EPI),
    ("fwd", "xbf_halo"): (HALO7 + (8,), (1, 2, 3), {"row": ({}, GHALO), "col": ({"colmajor": 0}, GHCOL)}, XBF_EPI),
    ("fwd", "xbf_halo3"): (HALO7 + (37,), (1, 2), {"taps9": ({}, GH3), "generic": ({}, GH3G)}, HALO3_EPI),
    ("fwd", "xbf_panel"): ((0, 1, 4, 17), (1, 2, 3), {"nbw3k2": (SMALL_PANEL, GPANEL(64, (192, 100, 37))),
                                                      "nbw3k3": (SMALL_PANEL, GPANEL(96, (192, 100, 37))),
                                                      "nbw1k6": (dict(SMALL_PANEL, panel_k192=1), GPANEL(192, (64, 40, 37)))}, XBF_EPI),
    ("wgrad", "f32_tile"): (WG8, (0,), {"": ({}, G33[:3])}, WG_EPI + WG_PS_EPI[:2]),
    ("wgrad", "xbf_tile"): (WG8, (1, 2, 3), {"dy": ({}, G33[:3]), "dy_ps": ({}, G33[:2])}, None),
    ("wgrad", "xbf_3k"): ((0, 1), (1, 2), {"": ({}, [(1, 4, 16, 64, 64, 3, 3, 1, 1), (3, 5, 13, 64, 40, 3, 3, 1, 1), (2, 3, 7, 192, 37, 1, 1, 0, 0)])}, WG3_EPI),
    ("wgrad", "xbf_halo"): (HALO7, (1, 2, 3), {"ne7": ({}, [(1, 2, 64, 128, 128, 3, 3, 1, 1), (2, 3, 30, 128, 136, 3, 3, 1, 1)]),
                                               "ne9": ({}, [(1, 4, 80, 128, 128, 3, 3, 1, 1)])}, WGH_EPI),
    ("batch", "batch"): ((0, 1, 3), (1, 2, 3), {"": ({}, [(2, 1, 26, 64, 40, 1, 1, 0, 0), (3, 1, 7, 32, 72, 1, 1, 0, 0)])}, BATCH_EPI),
}
CLASS_EPI = {("wgrad", "xbf_tile", "dy"): WG_EPI, ("wgrad", "xbf_tile", "dy_ps"): WG_PS_EPI}
PANEL_NBW = {"nbw3k2": 3, "nbw3k3": 3, "nbw1k6": 1}
WGH_NE = {"ne7": 7, "ne9": 9}
RUNTIME_LOADER = (("fwd", "f32_scalar"), ("wgrad", "f32_scalar"))

# the scalar kernels: (ld, geometry, epilogue); Cin 1 and 3, a concat over 6 channels, and vector-width channels with unaligned rows
SCALAR_FWD = [(0, (1, 4, 16, 1, 64, 3, 3, 1, 1), ()), (1, (3, 5, 13, 1, 40, 3, 3, 1, 1), ("bias", "bn")), (2, (2, 3, 7, 3, 37, 1, 1, 0, 0), ("bias", "relu")),
              (3, (3, 5, 13, 3, 40, 3, 3, 1, 1), ("bias",)), (4, (1, 4, 16, 3, 64, 3, 3, 1, 1), ("outwin", "bias")), (5, (2, 6, 9, 3, 72, 2, 2, 0, 0), ("bias", "ps")),
              (7, (3, 5, 13, 3, 40, 3, 3, 1, 1), ("bn",)), (8, (3, 5, 13, 4, 37, 3, 3, 1, 1), ("bias", "tanh")), (17, (2, 3, 7, 6, 37, 1, 1, 0, 0), ("bias",)),
              (16, (3, 5, 13, 6, 40, 3, 3, 1, 1), ("stride", "bias")), (0, (2, 3, 7, 3, 40, 1, 3, 0, 1), ("dil", "bn")), (0, (2, 3, 7, 3, 40, 1, 1, 0, 0), ("inwin",))]
SCALAR_WG = [(0, (1, 4, 16, 1, 64, 3, 3, 1, 1), ("z",)), (1, (3, 5, 13, 1, 40, 3, 3, 1, 1), ("db",)), (3, (3, 5, 13, 3, 40, 3, 3, 1, 1), ("db", "z")),
             (4, (2, 3, 7, 3, 37, 1, 1, 0, 0), ("db",)), (7, (2, 6, 9, 3, 72, 2, 2, 0, 0), ("dyps",)), (2, (3, 5, 13, 16, 37, 3, 3, 1, 1), ("db", "rawdy")),
             (17, (2, 3, 7, 6, 40, 1, 1, 0, 0), ("db", "dywin")), (8, (3, 5, 13, 4, 37, 3, 3, 1, 1), ("db", "rawdy"))]

# (kernel, ld, epilogue) of the engines' recorded launches (tests/golden/conv_routes.json) beyond what the rotation lands on; added for every T
RECORDED = {
    ("fwd", "f32_tile"): [(0, ("bias", "bn")), (0, ("bias", "ps")), (0, ("bias", "wtwin")), (0, ("bn", "dil")), (0, ("wtwin",)), (0, ("wtwin", "stride")), (0, ()),
                          (3, ("bias",)), (3, ("bias", "bn")), (3, ("bn",)), (3, ("bn", "dil")), (4, ("bias",)), (5, ("bias", "ps")), (8, ()), (17, ("bias",))],
    ("fwd", "f32_wstat"): [(0, ("bias", "bn"))],
    ("fwd", "xbf_halo"): [(0, ("bias", "bn")), (0, ("bias", "ps")), (0, ("bnb1",)), (0, ("bnb2",)), (0, ("bias",)), (3, ("bias",)), (5, ("bias", "ps")), (8, ("bnb0",)), (8, ())],
    ("fwd", "xbf_halo3"): [(0, ("bias", "bn", "rt3")), (0, ("bias", "ps")), (0, ("bnb1", "rt3")), (0, ("bnb2", "rt3")), (0, ("bias",)), (3, ("bias",))],
    ("fwd", "xbf_tile"): [(0, ("bias", "bn")), (0, ("bn", "dil")), (0, ("bnb0", "wtwin")), (0, ("bnb1",)), (0, ("bnb1", "wtwin")), (0, ("bnb1", "wtwin", "stride")),
                          (0, ("dzonly",)), (0, ("wtwin",)), (0, ("wtwin", "stride")), (0, ("bias", "wtwin")), (0, ("bias",)),
                          (3, ("bias",)), (3, ("bias", "bn")), (3, ("bn",)), (3, ("bn", "dil"))],
    ("fwd", "xbf_splitk"): [(0, ("bias", "bn")), (0, ("bnb1", "wtwin", "stride")), (3, ("bn", "dil"))],
    ("wgrad", "f32_tile"): [(0, ("db",)), (0, ("db", "dyps", "z")), (0, ("db", "dywin")), (0, ("db", "dywin", "inwin")), (0, ("db", "z")), (0, ("dil",)), (0, ("z",)),
                            (3, ()), (3, ("db", "dywin")), (3, ("db", "z")), (3, ("dil",)), (4, ("db",)), (5, ("db", "dyps", "z")), (17, ("db",))],
    ("wgrad", "xbf_tile"): [(0, ("db",)), (0, ("db", "dyps", "z")), (0, ("db", "dywin")), (0, ("db", "dywin", "inwin")), (0, ("db", "z")), (0, ("dil",)), (0, ("z",)),
                            (3, ()), (3, ("db", "dywin")), (3, ("db", "z")), (3, ("dil",)), (5, ("db", "dyps", "z"))],
    ("wgrad", "xbf_3k"): [(0, ("db", "z")), (0, ("z",))],
}


def r4(n):
    return (n + 3) // 4 * 4


class MCase:
    def __init__(self, op, kernel, T, ld, cls, geom, flags, knobs, idx):
        self.op, self.kernel, self.T, self.ld, self.cls, self.flags, self.knobs, self.idx = op, kernel, T, ld, cls, tuple(flags), dict(knobs), idx
        g = tuple(geom) + (1, 1, 0, 0)[len(geom) - 5:] if len(geom) < 9 else tuple(geom)
        self.N, self.H, self.Wr, self.Cin, self.Cout, self.KH, self.KW, self.ph, self.pw = g
        f = self.flags
        self.dil, self.sw = (2 if "dil" in f else 1), (2 if "stride" in f else 1)
        self.W = (self.Wr - 1) * self.dil + 1                       # logical (zero-dilated) width
        self.OH = self.H + 2 * self.ph - self.KH + 1
        self.OW = (self.W + 2 * self.pw - self.KW) // self.sw + 1
        self.M, self.K = self.N * self.OH * self.OW, self.KH * self.KW * self.Cin
        self.Ca = self.Cin // 2 if ld & 16 else self.Cin            # channels of `in` (the rest: the strip)
        if ld & 16 and self.Ca % 4:
            self.Ca = 4
        self.in_ld, self.in_coff = (self.Ca + 8, 4) if "inwin" in f else (self.Ca, 0)
        wcols = r4(self.Cout)
        self.wt_ld, self.wt_coff = (wcols + 36, 32) if "wtwin" in f else ((wcols, 0) if wcols != self.Cout else (0, 0))
        if kernel == "f32_scalar" and op == "fwd" and ld == 8:
            self.wt_ld, self.wt_coff = self.Cout + 2, 1             # unaligned weight rows: the scalar kernel's with a vector-width Cin
        self.out_ld, self.out_coff = (wcols + 8, 4) if "outwin" in f else (self.Cout, 0)
        if "rawdy" in f:
            self.dy_ld, self.dy_coff = self.Cout, 0                 # rows of an odd length: no vector loads of dy
        else:
            self.dy_ld, self.dy_coff = (wcols + 8, 4) if "dywin" in f else (wcols, 0)
        self.rt = 3 if "rt3" in f else 1
        self.bnb = next((x for x in ("bnb0", "bnb1", "bnb2", "dzonly") if x in f), None)
        self.bnb_act = {None: None, "bnb0": "none", "bnb1": "relu", "bnb2": "mish", "dzonly": "mish"}[self.bnb]
        self.stats = ("sdz", "sdzx") if self.bnb and self.bnb != "dzonly" else (("sum", "sumsq") if "bn" in f else ())
        small = self.N * self.H * self.Wr * self.Cin <= 8192
        self.act = None if not ld & 2 else ("relu" if (idx % 2 and small) else "mish")
        self.out_act = "relu" if "relu" in f else "tanh" if "tanh" in f else None
        self.splits = 0
        if kernel == "xbf_splitk":
            self.splits = 2 + idx % 2 if self.kp // 32 >= 3 else 2
        if op != "fwd":
            tiles = (self.M + 63) // 64
            self.splits = min(tiles, 2 + idx % 2) if ("z" in f or kernel == "xbf_halo") else 0
            if self.splits:                                         # no empty split: whole 64-pixel tiles per split
                self.splits = -(-tiles // -(-tiles // self.splits))
        self.mate = None
        self.id = f"{op}-{kernel}-T{T}-ld{ld}-{cls or 'x'}-{idx}-" + ("+".join(f) or "plain")
        self.seed = 0
        # what kernel_table.bound_of reads
        self.scalars, self.extra, self._extra, self.caps = (), {}, {}, {}

    @property
    def kp(self):
        return (self.K + 31) // 32 * 32

    @property
    def xbf(self):
        return self.T > 0 and self.Cin % 4 == 0

    @property
    def policy(self):
        return POLICY[self.T]

    @property
    def keys(self):
        if self.op == "fwd":
            return ("out",) + self.stats
        return ("dw", "db") if "db" in self.flags else ("dw",)


def _compatible(kernel, ld, flags, geom):
    Cout = geom[4]
    f = set(flags)
    if ("ps" in f or "dyps" in f) and Cout % 4:
        return False
    if "ps" in f and kernel == "xbf_halo3" and ld & 4:          # the route leaves that pair to the two-workgroup kernel
        return False
    if ("inwin" in f or "dil" in f) and ld & 8:
        return False
    if ld & 8 and geom[3] % 4:
        return False
    if kernel == "xbf_splitk" and ((geom[5] if len(geom) > 5 else 1) * (geom[6] if len(geom) > 6 else 1) * geom[3] + 31) // 32 < 2:
        return False
    return True


def _table():
    cases = []
    for (op, kernel), (lds, terms, classes, epis) in KERNELS.items():
        for T in terms:
            # one slot per (shape class, loader variant); the epilogue classes rotate over the slots (more slots where a kernel has more
            # epilogue classes than variants), then the recorded (loader, epilogue) pairs on the first class
            parts = [([cls], CLASS_EPI[(op, kernel, cls)]) for cls in classes] if (op, kernel, next(iter(classes))) in CLASS_EPI else [(list(classes), epis)]
            idx = 0
            for pi, (clss, E) in enumerate(parts):
                slots = [(cls, ld) for cls in clss for ld in lds]
                todo = [slots[i % len(slots)] + (E[(i + T) % len(E)],) for i in range(max(len(slots), len(E)))]
                if pi == 0:
                    todo += [(clss[0], ld, fl) for ld, fl in RECORDED.get((op, kernel), [])]
                for i, (cls, ld, flags) in enumerate(todo):
                    knobs, geoms = classes[cls]
                    pick = None
                    for j in range(len(E) + 1):                  # the next epilogue / geometry this loader and kernel can take
                        fl = flags if j == 0 else E[(i + T + j) % len(E)]
                        for k in range(len(geoms)):
                            g = geoms[(i + k) % len(geoms)]
                            if _compatible(kernel, ld, fl, g):
                                pick = (fl, g)
                                break
                        if pick:
                            break
                    assert pick, (kernel, ld, flags)
                    c = MCase(op, kernel, T, ld, cls, pick[1], pick[0], knobs, idx)
                    if op == "batch":
                        c.mate = MCase(op, kernel, T, ld, cls, geoms[(i + 1) % len(geoms)], pick[0], knobs, idx + 100)
                    cases.append(c)
                    idx += 1
    for i, (ld, g, flags) in enumerate(SCALAR_FWD):
        cases.append(MCase("fwd", "f32_scalar", 0, ld, "", g, flags, {}, i))
    for i, (ld, g, flags) in enumerate(SCALAR_WG):
        cases.append(MCase("wgrad", "f32_scalar", 0, ld, "", g, flags, {}, i))
    ids = [c.id for c in cases]
    assert len(set(ids)) == len(ids), [x for x in ids if ids.count(x) > 1][:4]
    return cases


CASES = _table()
GROUPS = sorted({(c.op, c.kernel, c.T) for c in CASES})


def group(op, kernel, T):
    return [c for c in CASES if (c.op, c.kernel, c.T) == (op, kernel, T)]


# ---- operands ----------------------------------------------------------------------------------------------------------------------
def _act(v, name):
    if name in (None, "none"):
        return v
    if name == "relu":
        return torch.relu(v)
    if name == "tanh":
        return torch.tanh(v)
    return v * torch.tanh(F.softplus(v))


def _act_grad(z, name):
    if name == "none":
        return torch.ones_like(z)
    if name == "relu":
        return (z > 0).to(z.dtype)
    t = torch.tanh(F.softplus(z))
    return t + z * (1 - t * t) * torch.sigmoid(z)          # d/dz z tanh(softplus z)


def make(case, seed):
    """the case's operands: fp32 CPU tensors in the logical layout (N, H, Wr, C) / (M, C); `stored(case, d)` lays them out for the kernels"""
    c, g = case, _gen("conv_matrix", case.id, seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    d = {"x": rn(c.N, c.H, c.Wr, c.Ca)}
    if c.ld & 16:
        d["strip"] = rn(c.N, c.Wr, c.Cin - c.Ca)
    if c.ld & 1:
        d["sc"], d["sh"] = torch.rand(c.Cin, generator=g) + 0.5, rn(c.Cin) * 0.3
    if c.ld & 4:
        d["x2"] = rn(c.N, c.H, c.Wr, c.Cin)
    if c.ld & 32:
        d["s2"] = torch.rand(c.Cin, generator=g) + 0.5
    if c.op == "fwd":
        d["w"] = rn(c.K, c.Cout) / math.sqrt(c.K)
        if "bias" in c.flags:
            d["bias"] = rn(c.Cout)
        if c.bnb:
            y = rn(c.M, c.Cout) * 1.5 + 0.3
            d["mean"], d["rstd"] = rn(c.Cout) * 0.2 + 0.3, torch.rand(c.Cout, generator=g) + 0.4
            if c.bnb != "dzonly":
                d["bsc"], d["bsh"] = torch.rand(c.Cout, generator=g) + 0.5, rn(c.Cout) * 0.3
            if c.bnb_act == "relu":      # keep y * scale + shift away from the kink (too many elements for a seed to do it)
                z = y.double() * d["bsc"].double() + d["bsh"].double()
                near = z.abs() < 4 * RELU_MARGIN
                y = torch.where(near, ((torch.where(z < 0, -1.0, 1.0) * 8 * RELU_MARGIN - d["bsh"].double()) / d["bsc"].double()).float(), y)
            d["y"] = y
    else:
        d["dy"] = rn(c.M, c.Cout)
    return d


def operands(case):
    """the case's operands at the first seed of POOL_SEEDS that keeps the ReLU margin (seed 0 first)"""
    if getattr(case, "_ops", None) is None:
        for seed in (0,) + POOL_SEEDS:
            d = make(case, seed)
            if margin_of(case, d) > RELU_MARGIN:
                case.seed, case._ops = seed, d
                break
        else:
            raise AssertionError(f"{case.id}: no seed keeps the ReLU margin")
    return case._ops


def margin_of(case, d):
    m = float("inf")
    if case.act == "relu":
        z = d["x"].double()
        if case.ld & 1:
            z = z * d["sc"][:case.Ca].double() + d["sh"][:case.Ca].double()
        m = min(m, z.abs().min().item())
    if case.bnb_act == "relu":
        m = min(m, (d["y"].double() * d["bsc"].double() + d["bsh"].double()).abs().min().item())
    return m


# ---- references ----------------------------------------------------------------------------------------------------------------------
def loader(case, d, dt):
    """the A operand after the fused prologue, logical [N][Cin][H][W] (zero-dilated), in dtype dt"""
    c = case
    v = d["x"].to(dt)
    if c.ld & 1:
        v = v * d["sc"][:c.Ca].to(dt) + d["sh"][:c.Ca].to(dt)
    if c.ld & 2:
        v = _act(v, c.act)
    if c.ld & 32:
        v = v + d["x2"].to(dt) * d["s2"].to(dt)
    elif c.ld & 4:
        v = v + d["x2"].to(dt)
    if c.ld & 16:
        v = torch.cat([v, d["strip"].to(dt)[:, None].expand(c.N, c.H, c.Wr, c.Cin - c.Ca)], -1)
    if c.dil > 1:
        z = v.new_zeros(c.N, c.H, c.W, c.Cin)
        z[:, :, ::c.dil] = v
        v = z
    return v.permute(0, 3, 1, 2).contiguous()


def _cols(case, a):
    """im2col of the logical input: [M][K], k = (kh KW + kw) Cin + ci"""
    c = case
    u = F.unfold(a, (c.KH, c.KW), padding=(c.ph, c.pw), stride=(1, c.sw))          # [N][Cin KH KW][OH OW]
    assert u.shape[-1] == c.OH * c.OW, (c.id, u.shape)
    return u.view(c.N, c.Cin, c.KH * c.KW, -1).permute(0, 3, 2, 1).reshape(c.M, c.K)


def split_terms(x32, T):
    """x1 = bf16(x), x2 = bf16(x - x1), x3 = bf16(x - x1 - x2) of an fp32 tensor, each as float64; T = 0: the tensor itself"""
    assert x32.dtype == F32
    if T == 0:
        return [x32.double()]
    out, r = [], x32
    for _ in range(T):
        h = r.bfloat16().float()
        out.append(h.double())
        r = r - h
    return out


def _product(A, B, T, dt):
    """sum over the kept term pairs of A_i^T-free product: A [m][k] terms x B [k][n] terms"""
    if T == 0 or dt != F64:
        return A[0] @ B[0]
    acc = 0
    for i in range(T):      # i + j <= T + 1 (1-based): a_i meets b_1 .. b_(T - i)
        acc = acc + A[i] @ sum(B[:T - i])
    return acc


def _blocks(t, rows):
    pad = (-t.shape[0]) % rows
    return torch.cat([t, t.new_zeros(pad, t.shape[1])]).reshape(-1, rows, t.shape[1]).sum(1)


def evaluate(case, d, *, T=None, loader_dt=F64, dt=F64, nudge=0):
    """every key of the case.  T = None: the truth (dt = F64) or its float32 restatement (dt = F32, loader in float32 too).
    T = 0 .. 3: the T-term model in float64, over the loader evaluated in loader_dt and rounded to fp32 (nudge = +-1: moved one ulp)"""
    c = case
    if T is None:
        a = loader(c, d, dt)
        A = [_cols(c, a)]
        cast = lambda t: [t.to(dt)]
        TT = 0
    else:
        a32 = loader(c, d, loader_dt).float()
        if nudge:
            a32 = torch.where(a32 == 0, a32, torch.nextafter(a32, torch.full_like(a32, float("inf") * nudge)))      # (padding stays zero)
        A = [_cols(c, t) for t in split_terms(a32, T)]
        cast = lambda t: split_terms(t, T)
        TT = T
    res = {}
    if c.op == "fwd":
        raw = _product(A, cast(d["w"]), TT, dt)                                        # [M][Cout]
        if c.bnb:
            y = d["y"].to(dt)
            sc, sh = (d["bsc"].to(dt), d["bsh"].to(dt)) if "bsc" in d else (1.0, 0.0)
            dz = raw * _act_grad(y * sc + sh, c.bnb_act)
            if c.stats:
                res["sdz"] = _blocks(dz, 64 * c.rt)
                res["sdzx"] = _blocks(dz * (y - d["mean"].to(dt)) * d["rstd"].to(dt), 64 * c.rt)
            res["out"] = dz if ("dz" in c.flags or c.bnb == "dzonly") else raw
        else:
            if c.stats:
                res["sum"], res["sumsq"] = _blocks(raw, 64 * c.rt), _blocks(raw * raw, 64 * c.rt)
            pre = raw + d["bias"].to(dt) if "bias" in d else raw
            res["out"] = _act(pre, c.out_act)
            if T is None and dt == F64 and c.out_act:
                c._act_scale = max(1.0, pre.abs().max().item() / res["out"].abs().max().item())
    else:
        Y = cast(d["dy"])
        res["dw"] = _product([t.t() for t in A], Y, TT, dt)                            # [K][Cout]
        if "db" in c.flags:
            # the tile loops add the fp32 dy; the halo kernel reads dy through its pre-split planes only and forms the bias gradient on the
            # matrix cores as the product 1 * dy (csrc/conv_xbf.hip: accdb): a = 1 has one term, so the kept products are dy_1 .. dy_T
            res["db"] = sum(Y).sum(0) if (T is not None and c.kernel == "xbf_halo") else d["dy"].to(dt).sum(0)
    return res


def references(case):
    """(truth, ref32, model, d_loader, d_ulp) of the case, computed once"""
    if getattr(case, "_refs", None) is None:
        d = operands(case)
        truth, ref32 = evaluate(case, d), evaluate(case, d, dt=F32)
        model = evaluate(case, d, T=case.T)
        arithmetic = bool(case.ld & (1 | 2 | 4 | 32))
        zero = {k: 0.0 for k in model}
        if arithmetic:
            m32 = evaluate(case, d, T=case.T, loader_dt=F32)
            d_loader = {k: err(m32[k], model[k]) for k in model}
            up, dn = evaluate(case, d, T=case.T, nudge=1), evaluate(case, d, T=case.T, nudge=-1)
            d_ulp = {k: max(err(up[k], model[k]), err(dn[k], model[k])) for k in model}
        else:
            d_loader, d_ulp = zero, dict(zero)
        case._refs = (truth, ref32, model, d_loader, d_ulp)
    return case._refs


def bounds(case):
    """key -> (bound against the truth, bound against the model)"""
    truth, ref32, model, d_loader, d_ulp = references(case)
    val, par = limits(case.policy)
    out = {}
    for k in case.keys:
        extra = 4 * d_loader[k] + 4 * d_ulp[k]
        if k in FWD_STATS:
            mult = 8 if k in ("sdz", "sdzx") else 4
            case.caps = {k: STAT_CAP if mult == 4 else 8 * MODEL_LIMITS[0]}
            m32 = {k: ref32[k]}
            b, _ = bound_of(case, k, m32, {k: truth[k]})               # 4 e_ref32 + FLOOR, capped
            out[k] = (mult * val, b + extra)
        else:
            lim, mlim = (val, MODEL_LIMITS[0]) if k == "out" else (par, MODEL_LIMITS[1])
            if k == "out" and case.out_act:
                lim *= case._act_scale
            out[k] = (lim, mlim + extra)
    return out


def check_well_posed(case):
    """CPU: sizes, margins, finite references with every key, finite d_loader / d_ulp / e_ref32, and the float32-CPU reference inside every bound"""
    d = operands(case)
    assert all(v.numel() * 4 <= SIZE_LIMIT and v.dtype == F32 for v in d.values()), case.id
    assert case.M * max(case.out_ld, case.Cout) * 4 <= SIZE_LIMIT and case.splits * case.K * case.Cout * 4 <= SIZE_LIMIT, case.id
    if case.act == "relu" or case.bnb_act == "relu":
        assert margin_of(case, d) > RELU_MARGIN, case.id
    truth, ref32, model, d_loader, d_ulp = references(case)
    assert set(truth) == set(ref32) == set(model) == set(case.keys), (case.id, sorted(truth))
    B = bounds(case)
    for k in case.keys:
        assert truth[k].dtype == F64 and model[k].dtype == F64 and ref32[k].dtype == F32, (case.id, k)
        assert torch.isfinite(truth[k]).all() and torch.isfinite(model[k]).all() and truth[k].abs().max() > 0, (case.id, k)
        e32, em = err(ref32[k], truth[k]), err(ref32[k], model[k])
        assert all(math.isfinite(v) for v in (e32, d_loader[k], d_ulp[k], B[k][0], B[k][1])), (case.id, k)
        assert e32 <= B[k][0], (case.id, k, "float32 CPU reference against the truth", e32, B[k][0])
        if case.T in (0, 3):     # (the float32 reference computes the unsplit product: only comparable with the models that keep it)
            assert em <= B[k][1], (case.id, k, "float32 CPU reference against the model", em, B[k][1])


# ---- argument blocks -----------------------------------------------------------------------------------------------------------------
OPERANDS = ("in", "in2", "sc", "sh", "s2", "strip", "wt", "wt_bf", "bias", "out", "part", "y", "mean", "rstd", "bsc", "bsh", "sk", "dy", "wpart", "dbpart", "dy_bf")


def fake_ptrs():
    return {n: PTR + 0x100000 * i for i, n in enumerate(OPERANDS)}


def block(case, P):
    """the ConvArgs (fwd) / WgradArgs (wgrad, batch) of the case over the operand addresses P"""
    from tpgsr_amd import _lib as L
    c, a = case, L.ConvArgs()
    a.in_ = P["in"]
    a.N, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW, a.pad_h, a.pad_w, a.OH, a.OW = c.N, c.H, c.W, c.Cin, c.Cout, c.KH, c.KW, c.ph, c.pw, c.OH, c.OW
    a.in_ld, a.in_coff, a.in2_ld, a.out_ld, a.out_coff = c.in_ld, c.in_coff, c.Cin, c.out_ld, c.out_coff
    a.in_dil_w, a.stride_w, a.wt_ld, a.wt_coff = c.dil, c.sw, c.wt_ld, c.wt_coff
    if c.ld & 1:
        a.in_scale, a.in_shift = P["sc"], P["sh"]
    if c.ld & 2:
        a.in_act = L.act_code(c.act)
    if c.ld & 4:
        a.in2 = P["in2"]
    if c.ld & 8:
        a.in_ps = 1
    if c.ld & 16:
        a.in_b, a.cin_a, a.in_b_ld = P["strip"], c.Ca, c.Cin - c.Ca
    if c.ld & 32:
        a.in2_scale = P["s2"]
    a.terms = c.T if c.Cin % 4 == 0 else 0
    if c.op == "fwd":
        a.wt, a.out = P["wt"], P["out"]
        if c.xbf:
            a.kp, a.wt_bf = c.kp, P["wt_bf"]
            a.wt_bf_cin = c.Cin if (c.Cin % 32 == 0 and c.KH * c.KW > 1) else 0           # (kernels.block_order_cin)
            a.sk_splits = c.splits if c.kernel == "xbf_splitk" else 1                     # 1: explicitly unsplit (0 is offered to the planner)
            if c.kernel == "xbf_splitk":
                a.sk_part = P["sk"]
        if "bias" in c.flags:
            a.bias = P["bias"]
        a.out_act, a.out_ps = L.act_code(c.out_act), int("ps" in c.flags)
        if c.stats:
            a.bn_partial = P["part"]
        if c.rt == 3:
            a.bn_row_tiles = 3
        if c.bnb:
            a.bnb_y, a.bnb_act, a.bnb_store_dz = P["y"], L.act_code(c.bnb_act), int("dz" in c.flags or c.bnb == "dzonly")
            if c.bnb != "dzonly":
                a.bnb_mean, a.bnb_rstd, a.bnb_scale, a.bnb_shift = P["mean"], P["rstd"], P["bsc"], P["bsh"]
        return a
    w = L.WgradArgs()
    w.c = a
    w.dy, w.dy_ld, w.dy_coff, w.dy_ps, w.part = P["dy"], c.dy_ld, c.dy_coff, int("dyps" in c.flags), P["wpart"]
    if "db" in c.flags:
        w.dbpart = P["dbpart"]
    w.zsplits = c.splits
    if c.kernel == "xbf_halo":
        w.dy_bf = P["dy_bf"]
    return w


class knobs:
    """``with knobs(case.knobs):`` sets the library's switches through their setters and restores the defaults"""

    def __init__(self, kn):
        self.kn = kn

    def __enter__(self):
        from tpgsr_amd import _lib as L
        self.lib = L.load()
        self.lib.tpgsr_halo_set_colmajor_min_bytes.argtypes = [C.c_longlong]
        self.lib.tpgsr_panel_set_min_m.argtypes = [C.c_longlong]
        for k, v in self.kn.items():
            getattr(self.lib, KNOBS[k][0])(v)
        return self.lib

    def __exit__(self, *exc):
        for k in self.kn:
            getattr(self.lib, KNOBS[k][0])(KNOBS[k][1])
        return False


def route_of(case, P=None):
    """(kernel name, route struct) of the case's block under its switches"""
    from tpgsr_amd import kernels as K
    with knobs(case.knobs):
        return K.conv_route(block(case, P or fake_ptrs()))


def expected_route(case):
    """the host-side launch parameters the case pins, next to (kernel, ld)"""
    c, want = case, {}
    if c.op == "fwd":
        want["nbw"] = PANEL_NBW.get(c.cls, 0) if c.kernel == "xbf_panel" else 0
        want["splits"] = c.splits if c.kernel == "xbf_splitk" else 0
    else:
        want["ne"] = WGH_NE.get(c.cls, 0) if c.kernel == "xbf_halo" else 0
        if c.splits:
            want["Z"] = c.splits
        want["vecY"] = 0 if ("rawdy" in c.flags or "dyps" in c.flags) else 1
    return want


def assert_route(case, P=None):
    name, r = route_of(case, P)
    want_kernel = "xbf_tile" if case.op == "batch" else case.kernel
    assert (name, r.ld) == (want_kernel, case.ld), f"{case.id}: routed to {name}<{r.ld}>, the table says {want_kernel}<{case.ld}>"
    for k, v in expected_route(case).items():
        assert getattr(r, k) == v, f"{case.id}: route.{k} = {getattr(r, k)}, the table says {v}"
    if case.op == "fwd" and case.rt == 3:
        from tpgsr_amd import _lib as L
        with knobs(case.knobs):
            assert L.load().tpgsr_conv_bn_row_tiles(C.byref(block(case, P or fake_ptrs()))) == 3, case.id
    return name, r


# ---- the GPU side --------------------------------------------------------------------------------------------------------------------
def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def stored(case, d):
    """device tensors in the layouts the kernels read, + the pre-filled outputs; returns (tensors, addresses)"""
    from tpgsr_amd import kernels as K
    c, g = case, _gen("conv_matrix_fill", case.id)
    t = {}
    if c.ld & 8:        # stored pixel-shuffled [N][2H][2W][Cin / 4]
        xs = F.pixel_shuffle(d["x"].permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).contiguous()
        t["in"] = xs.reshape(-1, c.Cin // 4)
    else:
        buf = torch.randn(c.N * c.H * c.Wr, c.in_ld, generator=g)
        buf[:, c.in_coff:c.in_coff + c.Ca] = d["x"].reshape(-1, c.Ca)
        t["in"] = buf
    for k, n in (("x2", "in2"), ("sc", "sc"), ("sh", "sh"), ("s2", "s2"), ("strip", "strip"), ("bias", "bias"), ("y", "y"), ("mean", "mean"),
                 ("rstd", "rstd"), ("bsc", "bsc"), ("bsh", "bsh")):
        if k in d:
            t[n] = d[k].reshape(-1, d[k].shape[-1]) if d[k].dim() > 2 else d[k]
    if c.op == "fwd":
        wcols = c.wt_ld or c.Cout
        wbuf = torch.randn(c.K, wcols, generator=g) if c.wt_ld else None
        if wbuf is None:
            wbuf = d["w"].clone()
        else:
            wbuf[:, c.wt_coff:c.wt_coff + c.Cout] = d["w"]
        t["wt"] = wbuf
    else:
        if "dyps" in c.flags:
            dy4 = d["dy"].view(c.N, c.OH, c.OW, c.Cout).permute(0, 3, 1, 2)
            t["dy"] = F.pixel_shuffle(dy4, 2).permute(0, 2, 3, 1).contiguous().reshape(-1, c.Cout // 4)
        else:
            buf = torch.randn(c.M, c.dy_ld, generator=g)
            buf[:, c.dy_coff:c.dy_coff + c.Cout] = d["dy"]
            if c.dy_ld > c.dy_coff + c.Cout and "dywin" not in c.flags:
                buf[:, c.Cout:] = 0.0                         # rows padded to a multiple of four floats
            t["dy"] = buf
    t = {k: v.contiguous().to(DEV) for k, v in t.items()}
    if c.op == "fwd":
        if c.xbf:
            twin, kp = K.make_bf_twin(t["wt"], c.Cin)
            assert kp == c.kp and t["wt"]._tpgsr_twin[2] == (c.Cin if (c.Cin % 32 == 0 and c.KH * c.KW > 1) else 0), c.id
            t["wt_bf"] = twin
        t["out"] = _nan(4 * c.M + 4, c.Cout // 4) if "ps" in c.flags else _nan(c.M + 1, c.out_ld)
        if c.stats:
            t["part"] = _nan(K.bn_rows(c.M, c.rt) + 1, 2, c.Cout)
        if c.kernel == "xbf_splitk":
            t["sk"] = _nan(c.splits * ((c.M + 63) // 64) * ((c.Cout + 63) // 64) * 256 * 16)
    else:
        Z = route_of(c)[1].Z
        t["wpart"] = _nan(Z + 1, c.K, c.Cout)
        if "db" in c.flags:
            t["dbpart"] = _nan(Z + 1, c.Cout)
        if c.kernel == "xbf_halo":
            t["dy_bf"] = torch.zeros(3 * ((c.M + 15) // 16) * ((c.Cout + 31) // 32) * 1024, dtype=torch.uint8, device=DEV)
    return t, {k: v.data_ptr() for k, v in t.items()}


def unpack(case, t):
    """the launch's results as CPU tensors in the reference's layout, after checking that every pre-fill outside the results survived"""
    c, res = case, {}
    if c.op == "fwd":
        o = t["out"].cpu()
        if "ps" in c.flags:
            assert torch.isnan(o[4 * c.M:]).all(), f"{c.id}: guard rows behind the pixel-shuffled output written"
            o4 = o[:4 * c.M].view(c.N, 2 * c.OH, 2 * c.OW, c.Cout // 4).permute(0, 3, 1, 2)
            res["out"] = F.pixel_unshuffle(o4, 2).permute(0, 2, 3, 1).reshape(c.M, c.Cout)
        else:
            assert torch.isnan(o[c.M:]).all(), f"{c.id}: guard row behind the output written"
            win = o[:c.M, c.out_coff:c.out_coff + c.Cout]
            assert torch.isnan(o[:c.M, :c.out_coff]).all() and torch.isnan(o[:c.M, c.out_coff + c.Cout:]).all(), f"{c.id}: columns outside the output window written"
            res["out"] = win
        if c.stats:
            p = t["part"].cpu()
            assert torch.isnan(p[-1]).all(), f"{c.id}: guard row behind the statistics written"
            res[c.stats[0]], res[c.stats[1]] = p[:-1, 0], p[:-1, 1]
    else:
        p = t["wpart"].cpu()
        assert torch.isnan(p[-1]).all(), f"{c.id}: guard slab behind the splits written"
        res["dw"] = p[:-1].double().sum(0)
        if "db" in c.flags:
            b = t["dbpart"].cpu()
            assert torch.isnan(b[-1]).all(), f"{c.id}: guard row behind the bias-gradient splits written"
            res["db"] = b[:-1].double().sum(0)
    for k, v in res.items():
        assert not torch.isnan(v).any(), f"{c.id} {k}: {int(torch.isnan(v).sum())} elements never written"
    return res


def launch(case, t, P):
    """route asserted, then the launch (under the case's switches)"""
    from tpgsr_amd import kernels as K
    assert_route(case, P)
    with knobs(case.knobs):
        a = block(case, P)
        if case.op == "fwd":
            K.conv_fwd(a)
        else:
            K.conv_wgrad(a)
    torch.cuda.synchronize()


def run_gpu(case):
    t, P = stored(case, operands(case))
    launch(case, t, P)
    return unpack(case, t), t, P


def compare(case, got, worst, log=print):
    """every key element-wise under both references"""
    truth, ref32, model, d_loader, d_ulp = references(case)
    B = bounds(case)
    assert set(got) == set(case.keys), (case.id, sorted(got))
    bad = []
    for k in case.keys:
        assert tuple(got[k].shape) == tuple(truth[k].shape), (case.id, k, tuple(got[k].shape), tuple(truth[k].shape))
        et, em = err(got[k], truth[k]), err(got[k], model[k])
        bt, bm = B[k]
        w = worst.setdefault((case.op, case.kernel, case.T), {})
        for name, e, b in (("truth", et, bt), ("model", em, bm)):
            if e / b > w.get(name, (0.0,))[0]:
                w[name] = (e / b, e, b, case.id, k)
        log(f"{case.id} {k}: vs truth {et:.2e} / {bt:.2e}   vs model {em:.2e} / {bm:.2e}   (d_loader {d_loader[k]:.2e}, d_ulp {d_ulp[k]:.2e}, "
            f"e_ref32 {err(ref32[k], truth[k]):.2e})")
        if not (et <= bt and em <= bm):
            dm = (got[k].double() - model[k]).abs().reshape(-1)
            at = int(dm.argmax())
            bad.append(f"{case.id} {k}: vs truth {et:.3e} (bound {bt:.3e}), vs model {em:.3e} (bound {bm:.3e}); worst flat element {at}: got "
                       f"{got[k].reshape(-1)[at].item():.9g}, model {model[k].reshape(-1)[at].item():.9g}, truth {truth[k].reshape(-1)[at].item():.9g}")
    return bad
