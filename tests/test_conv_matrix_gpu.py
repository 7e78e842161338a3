"""GPU: every instantiated convolution kernel variant against float64, route asserted (tests/conv_matrix_common.py holds the case table, the
references and the bounds; tests/test_conv_matrix_cpu.py keeps the table complete).

A parametrised test is one (launcher, kernel, T) and loops over that kernel's loader variants and shape classes.  For every case
  * the route is asserted on the very argument block that is launched (kernel, ld, and the host parameters the case pins) -- a case that
    drifts to another kernel when a threshold moves fails instead of staying green;
  * every key (out / the statistics rows, dw / db) is compared element-wise with the float64 truth under the policy's limit AND with the
    T-term model under the x3 limit + 4 d_loader + 4 d_ulp (both terms from the references alone, printed per case);
  * outputs are pre-filled with NaN: every element of the result must have been written, and the guard row / columns / slab must not.
Bit-exact, where the design promises it: xbf_halo3 = xbf_halo (outputs; statistics at one row per 64 pixels), xbf_3k = xbf_tile with the
plain loader, a batch item = its single launch.

OBSERVED-5d (MI355X):
  576 cases, 309 distinct (launcher, kernel, ld, T, shape class) combinations -- forward f32_tile 29,
  f32_scalar 12, f32_wstat 7, xbf_tile 105, xbf_splitk 69, xbf_halo 75, xbf_halo3 50, xbf_panel 45; weight gradient f32_tile 24, f32_scalar 8,
  xbf_tile 84, xbf_3k 14, xbf_halo 42; batch 12 (two items each).  All pass; every parametrised test under 2.2 s (the two xbf_halo3 ones;
  the others under 0.4 s).  Worst e / bound per (kernel, T), against the truth | against the model:
    forward   f32_tile 0.10 | 0.22   f32_scalar 0.05 | 0.11   f32_wstat 0.18 | 0.38
              xbf_tile   T1 0.21 | 0.39   T2 0.39 | 0.36   T3 0.11 | 0.28      xbf_splitk T1 0.15 | 0.21   T2 0.34 | 0.69   T3 0.08 | 0.36
              xbf_halo   T1 0.15 | 0.33   T2 0.29 | 0.57   T3 0.13 | 0.37      xbf_halo3  T1 0.14 | 0.36   T2 0.32 | 0.40
              xbf_panel  T1 0.15 | 0.26   T2 0.27 | 0.35   T3 0.10 | 0.21
    wgrad     f32_tile 0.06 | 0.06   f32_scalar 0.04 | 0.04   xbf_3k T1 0.14 | 0.01   T2 0.31 | 0.02
              xbf_tile   T1 0.17 | 0.02   T2 0.38 | 0.07   T3 0.05 | 0.04      xbf_halo   T1 0.15 | 0.13   T2 0.31 | 0.07   T3 0.05 | 0.04
              batch      T1 0.16 | 0.01   T2 0.37 | 0.07   T3 0.03 | 0.03
  (the model column's worst rows are the statistics: sum dz * xhat behind mish at 4 e_ref32 + 4 * 2^-24 = 1.0e-6 .. 2.3e-6.)
  Bit-exact: 49 xbf_halo3 launches = xbf_halo (out, and the statistics rows at one row per 64 pixels), 15 xbf_3k launches = xbf_tile,
  every batch item = its single launch.
  Two things the first run showed, neither a kernel bug:
    * the halo weight gradient forms the bias gradient on the matrix cores as 1 * dy over its pre-split planes: at T = 1 its db is the sum
      of bf16(dy), 1.1e-3 .. 2.3e-3 from the fp32 sum the tile loops give (inside the bf16 policy's 2e-2, 230 x the model bound when the
      model said "fp32 sum").  The model now states db of that kernel as the T-term product with a = 1; against it 0 .. 7e-9.
    * behind tanh the x2 kernels were at 1.6e-5 .. 2.6e-5 of max |out| = 1 (xbf_halo3 2.61e-5, xbf_splitk 2.11e-5 > 2e-5) while
      3.5e-7 .. 1.7e-6 from the model: the policy limit is relative to the linear result, whose largest element is 7 there.  The limit for
      `out` is now scaled by max |pre-activation| / max |out| of the truth (1.4e-4 and 1.0e-4 for those two cases).
  Found and fixed on the way: tpgsr_conv_wgrad_batch_prepare accepted every tile-loop loader variant although the batch kernel is
  instantiated for {0, 1, 3} only (a batch of ld 2 / 4 / 5 / 7 / 17 items was refused at launch instead of going out singly); the set is
  now in csrc/conv_route.cpp and prepare declines the others.  tests/test_bnb_fuse_gpu.py's "row panel" shape ran on the tile loop (the
  K = 192 panel is behind a switch) and two of its "halo" / "tile loop" shapes on split-K (the planner takes them): asserted now, with the
  switches set so that the named family runs.
  Mutants (scratch build, not committed), through this module:
    A  a2 b1 dropped in conv_wgrad_xbf_kernel<3, 2> (and the batch kernel's body): every ld 3 / T 2 weight gradient moved -- xbf_tile dw
       1.3e-3 .. 2.3e-3 against model bounds of 1.5e-5 .. 2.1e-5 (six cases), batch dw 2.0e-3 / 2.5e-3 against 2.2e-5 / 2.4e-5; nothing else.
    B  in_shift indexed with channel c + 4 in conv_halo_xbf_kernel<5, T, 7>: every xbf_halo ld 5 case at every T -- out 0.11 .. 0.24,
       sum / sum dz 0.9 .. 1.5 against model bounds of 5e-6 .. 1.8e-5 -- and the four xbf_halo3 ld 5 cases through the bit-exact
       comparison with xbf_halo (all 2 359 296 outputs differ); nothing else.
    Both fail against the model bound; A would also have failed the truth bound at T = 2 (2e-5) but not a bf16-level one.
"""
import pytest
import torch

import conv_matrix_common as M

pytestmark = pytest.mark.gpu
WORST = {}
FAULTED = []          # a launch that raised (a HIP error): nothing more is started on the device by this module
IDS = [f"{op}-{k}-T{T}" for op, k, T in M.GROUPS]


def _twin_case(c, kernel, cls, flags, knobs):
    """the same operands on another route (for the bit-exact promises)"""
    alt = M.MCase(c.op, kernel, c.T, c.ld, cls, (c.N, c.H, c.Wr, c.Cin, c.Cout, c.KH, c.KW, c.ph, c.pw), flags, knobs, c.idx)
    alt.act, alt.splits, alt._ops, alt.seed = c.act, c.splits, M.operands(c), c.seed
    return alt


def _bit_exact_twin(c, got_t):
    """-> list of complaints"""
    if c.kernel == "xbf_halo3" and c.ld != 37:
        alt = _twin_case(c, "xbf_halo", "row", tuple(f for f in c.flags if f != "rt3"), {"halo3": 0})
        if M.route_of(alt)[0] != "xbf_halo":
            return []
    elif c.kernel == "xbf_3k" and c.ld == 0:
        alt = _twin_case(c, "xbf_tile", "dy", c.flags, {"wgrad3": 0})
    else:
        return []
    t2, P2 = M.stored(alt, M.operands(alt))
    M.launch(alt, t2, P2)
    bad = []
    keys = ["out"] + (["part"] if c.stats and c.rt == 1 else []) if c.op == "fwd" else ["wpart"] + (["dbpart"] if "db" in c.flags else [])
    for k in keys:
        same = torch.equal(got_t[k].nan_to_num(nan=-7.0), t2[k].nan_to_num(nan=-7.0))
        print(f"{c.id}: {k} bit-exact with {alt.kernel}: {same}")
        if not same:
            bad.append(f"{c.id}: {k} differs from {alt.kernel}'s at {int((got_t[k].nan_to_num(nan=-7.0) != t2[k].nan_to_num(nan=-7.0)).sum())} elements")
    return bad


def _batch(c):
    """the case and its mate as single launches, then as one batched launch: the same slabs bit for bit -> (results of the batched item, complaints)"""
    from tpgsr_amd import kernels as K
    singles = []
    for x in (c, c.mate):
        t, P = M.stored(x, M.operands(x))
        M.launch(x, t, P)
        singles.append(t)
    batched, ws = [], []
    for x in (c, c.mate):
        t, P = M.stored(x, M.operands(x))
        M.assert_route(x, P)
        batched.append(t)
        ws.append(M.block(x, P))
    K.conv_wgrad_batch(ws)
    torch.cuda.synchronize()
    bad = []
    for x, a, b in zip((c, c.mate), singles, batched):
        for k in ["wpart"] + (["dbpart"] if "db" in x.flags else []):
            if not torch.equal(a[k].nan_to_num(nan=-7.0), b[k].nan_to_num(nan=-7.0)):
                bad.append(f"{x.id}: batched {k} differs from the single launch")
    return M.unpack(c, batched[0]), M.unpack(c.mate, batched[1]), bad


@pytest.mark.parametrize("grp", M.GROUPS, ids=IDS)
def test_kernel_variants_vs_fp64(grp):
    assert not FAULTED, f"not run: {FAULTED[0]} raised in a launch before"
    try:
        bad = _run_group(grp)
    except RuntimeError:
        FAULTED.append("-".join(map(str, grp)))
        raise
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:30])


def _run_group(grp):
    bad = []
    for c in M.group(*grp):
        if c.op == "batch":
            got, got2, b = _batch(c)
            bad += b + M.compare(c, got, WORST) + M.compare(c.mate, got2, WORST)
            continue
        got, t, P = M.run_gpu(c)
        bad += M.compare(c, got, WORST)
        bad += _bit_exact_twin(c, t)
    return bad


def test_zz_report():
    print("worst e / bound per (launcher, kernel, T): against the truth | against the model")
    for key in sorted(WORST):
        w = WORST[key]
        print(f"  {key[0]:5s} {key[1]:10s} T={key[2]}: " + " | ".join(f"{n} {w[n][1]:.2e} / {w[n][2]:.2e} = {w[n][0]:.2f} ({w[n][3]} {w[n][4]})" for n in ("truth", "model") if n in w))
    assert all(v[0] <= 1.0 for w in WORST.values() for v in w.values())
