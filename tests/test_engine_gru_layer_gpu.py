"""GPU: engine.GruLayer -- the GruBlock of the fused TSRN / TSRN_TL plans (1x1 conv and nn.GRU's input projection as ONE composed operand
Wc = W_ih W_1, bc = W_ih b_1 + b_ih) -- one layer at a time against the reference's GruBlock (model/tsrn.py:491-508: Conv2d 1x1 followed
by torch.nn.GRU, bidirectional) in float64 on the CPU, element by element; and the two kernels only this layer calls, directly:
tpgsr_compose_bwd_program (the chain rule from dWc / dbc back to conv1 and weight_ih / bias_ih) and pack-program kinds 5 and 6 (Wc, bc).

Harness and references: tests/engine_layer_common.py (the engine's own GruLayer runs, eagerly).  Layers (Cin, U, Hd, axis, loader): gru2 and
gru1 of TSRN, gru1 of TSRN_TL (affine + text strip), and the same three at hidden_units = 64; maps 2x16x64 and 1x16x64 (the one-launch forward
applies at 32 units) and 2x5x7 (it does not; bounds-tested scans, ragged pixel chunks of the fused weight gradient); policies x3, x2, bf16, f32.
Branches (each test asserts the launch list it produced):
  forward    tpgsr_bigru_proj_fwd                      32 units, split operands, scan length 64 or 16 (a multiple of four sequences)
             tpgsr_conv_fwd + tpgsr_bigru_fwd          32 units otherwise          tpgsr_conv_fwd + tpgsr_bigru_fwd_u   64 units
  backward   tpgsr_bigru_bwd2, tpgsr_gru_wgrad, 3 x tpgsr_wgrad_reduce             32 units, split operands
             tpgsr_bigru_bwd[_u], 3 x (tpgsr_conv_wgrad, tpgsr_wgrad_reduce)       otherwise (f32 at 32 units; every policy at 64 units)
  then the data gradient (tpgsr_conv_fwd over wc_d) and tpgsr_compose_bwd_program.
Compared with e = max |got - ref64| / max |ref64|, every key: h, dx ([P][Cin], strip columns included), conv1.weight / bias, and the eight GRU
parameters.  Bounds: the suite's limits for Fh.bigru at these shapes (tests/test_functional_ops_gpu.py: CONV_LIMITS) -- x3 and f32 5e-6 for
values and dx, 1e-5 for parameter gradients; x2 2e-5 -- and 2e-2 under bf16 (terms = 1, as tests/test_conv_panel_gpu.py).  The direct kernel
tests use the `arith` rule: e <= 4 e_ref32 + 4 * 2^-24, e_ref32 from the same computation in float32 on the CPU.

OBSERVED on an MI355X, worst e / bound per policy (`test_zz_report` prints it), all tests passing:
  GruLayer                        x3 0.08   x2 0.84   bf16 0.35   f32 0.19
  upstream gradient in two parts  x3 0.06   x2 0.47   f32 0.08            two accumulating passes  x3 0.06   x2 0.47   f32 0.08
  (the two rows agree to two digits: the same four cases; their worst keys are h under x2 and dx under f32, which printed the same e (9.42e-06, 3.87e-07) however the
   upstream gradient was split and however often the arena accumulated, and conv1.weight under x3 at 5.8e-7 and 6.5e-7 of 1e-5)
  tpgsr_compose_bwd_program 0.22 (of 4 e_ref32 + 4 * 2^-24)              pack kinds 5 / 6 0.28
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import engine_layer_common as E  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = E.gru_cases()
BY_ID = {c.id: c for c in CASES}
WORST = {}


def _compare(case, got, ref, policy, tag, scale=1.0):
    lim = E.limits(policy)
    bad = []
    for key in ("h", "dx") + E.GRU_KEYS:
        assert tuple(got[key].shape) == tuple(ref[key].shape), (key, tuple(got[key].shape), tuple(ref[key].shape))
        r = ref[key] if key == "h" or scale == 1.0 else ref[key] * scale
        if key == "dx" and scale != 1.0:
            r = ref[key]                                 # (dx is overwritten by every pass, only the arena accumulates)
        bound = lim[0] if key in ("h", "dx") else lim[1]
        e = E.err(got[key], r)
        WORST[tag] = max(WORST.get(tag, 0.0), e / bound)
        print(f"{case.id} {tag} {key}: e {e:.2e}  bound {bound:.0e}  ratio {e / bound:.2f}")
        if not e <= bound:
            bad.append(f"{key}: e {e:.3e} > {bound:.0e}")
    assert not bad, f"{case.id} {tag}: " + "; ".join(bad)


def _assert_branch(case, policy, names, eng, d, passes=1):
    from tpgsr_amd import kernels as K
    assert names == case.expected_launches(policy, passes), names
    L = eng.layer
    pa = K.make_bigru_proj_args(K.make_conv_args(K.ConvGeom(case.N, case.H, case.W, case.Cin, 6 * case.Hd), d["x"], L.wc_f, None, bias=L.bc,
                                                 **case.loader_kwargs(d)), L.whh, L.bhh, case.axis, d["h"], d["gates"])
    assert K.bigru_proj_supported(pa, case.Hd) == case.fused_forward(policy)
    assert K.gru_wgrad_fused(case.Hd) == case.fused_wgrad(policy)


@pytest.mark.parametrize("policy", E.POLICIES)
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_gru_layer_vs_fp64(case, policy):
    with E.conv_prec(policy):
        got, names, eng, d = E.run_gru(case, DEV)
        _assert_branch(case, policy, names, eng, d)
    _compare(case, got, case.reference(), policy, policy)


# one case per backward branch: fused weight gradient (32 units, split operands), unfused at 32 units (f32), the 64-unit scans
BRANCHES = [("C64-U64-axis0-residual-2x5x7", "x3"), ("C96-U64-axis1-affine+strip-1x16x64", "x2"), ("C64-U64-axis1-affine-2x5x7", "f32"),
            ("C160-U128-axis1-affine+strip-2x5x7", "x3")]


@pytest.mark.parametrize("cid,policy", BRANCHES)
def test_upstream_gradient_in_two_tensors(cid, policy):
    """dh + dh2 (the engine's two gradient paths into a block) against the reference of their sum"""
    case = BY_ID[cid]
    with E.conv_prec(policy):
        got, names, eng, d = E.run_gru(case, DEV, split_dh=True)
        _assert_branch(case, policy, names, eng, d)
    _compare(case, got, case.reference(), policy, policy + " dh+dh2")


@pytest.mark.parametrize("cid,policy", BRANCHES)
def test_two_backward_passes_accumulate(cid, policy):
    """bwd + flush_compose_bwd twice on one gradient arena: every parameter gradient is 2 x the reference (the += of the slab reduces and
    of the chain rule)"""
    case = BY_ID[cid]
    with E.conv_prec(policy):
        got, names, eng, d = E.run_gru(case, DEV, passes=2)
        _assert_branch(case, policy, names, eng, d, passes=2)
    _compare(case, got, case.reference(), policy, policy + " two passes", scale=2.0)


# ---- tpgsr_compose_bwd_program, directly ----------------------------------------------------------------------------------------
def _compose_launch(shapes):
    """one launch over `shapes`; every output pre-filled; -> per descriptor {name: tensor on the CPU}"""
    from tpgsr_amd import _lib, kernels as K
    lib = _lib.load()
    arr = (_lib.ComposeBwdDesc * len(shapes))()
    keep, outs, blk = [], [], 0
    for d, (Cin, U, G) in zip(arr, shapes):
        t, fill, _r64, _r32 = E.compose_case(Cin, U, G)
        dev = {k: v.to(DEV).contiguous() for k, v in {**t, **fill}.items()}
        for k, v in dev.items():
            setattr(d, k, v.data_ptr())
        d.Cin, d.U, d.G, d.blk0 = Cin, U, G, blk
        blk += lib.tpgsr_compose_bwd_blocks(Cin, U, G)
        keep.append(dev)
        outs.append({k: dev[k] for k in E.COMPOSE_OUT})
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    K.compose_bwd_program(table, len(shapes), blk)
    torch.cuda.synchronize()
    return [{k: v.cpu() for k, v in o.items()} for o in outs], blk


def test_compose_bwd_program_vs_fp64_autograd():
    """four descriptors of different shapes in one launch (segment boundaries inside workgroups; the last one's four segments in ONE workgroup),
    outputs pre-filled: += the float64 autograd of Wc = [W_ih0; W_ih1] W_1, bc = W_ih b_1 + b_ih; one descriptor alone gives the same bits"""
    from tpgsr_amd import _lib
    lib = _lib.load()
    assert lib.tpgsr_compose_bwd_blocks(4, 4, 3) == 1
    got, blk = _compose_launch(E.COMPOSE_SHAPES)
    assert blk == sum(lib.tpgsr_compose_bwd_blocks(*s) for s in E.COMPOSE_SHAPES)
    for shape, g in zip(E.COMPOSE_SHAPES, got):
        _t, _fill, r64, r32 = E.compose_case(*shape)
        for k in E.COMPOSE_OUT:
            e, bound = E.err(g[k], r64[k]), E.arith_bound(r32[k], r64[k])
            WORST["compose_bwd"] = max(WORST.get("compose_bwd", 0.0), e / bound)
            print(f"compose_bwd {shape} {k}: e {e:.2e}  bound {bound:.2e}  ratio {e / bound:.2f}")
            assert e <= bound, (shape, k, e, bound)
    for i, shape in enumerate(E.COMPOSE_SHAPES):
        alone, _ = _compose_launch([shape])
        for k in E.COMPOSE_OUT:
            assert torch.equal(alone[0][k], got[i][k]), (shape, k)


# ---- pack program kinds 5 and 6, directly ---------------------------------------------------------------------------------------
FILL = -7.0


def test_pack_kinds_5_and_6_vs_fp64():
    """Wc / bc of three GruBlocks, both directions into one [Cin][2G] / [2G][Cin] / [2G] operand each (GruLayer.__init__'s layout), in one
    program with a plain copy (kind 2) and a tiled kind-0 descriptor in between, so blk0 crosses kinds; cells nobody owns keep their fill"""
    from tpgsr_amd import _lib, kernels as K
    lib = _lib.load()
    shapes = [(64, 64, 96), (96, 64, 96), (160, 128, 192)]
    arr = (_lib.PackDesc * (4 * len(shapes) + 2))()      # per shape and direction one kind 5 and one kind 6; the copy; the tiled kind 0
    keep, want, extra, blk, i = [], [], {}, 0, 0

    def add(**f):
        nonlocal blk, i
        d = arr[i]
        i += 1
        for k, v in f.items():
            setattr(d, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
        d.wscale, d.blk0 = 1.0, blk
        blk += lib.tpgsr_pack_blocks(d.kind, d.Cout, d.Cin, d.KH, d.KW, d.numel)

    g = E._gen("pack56-neighbours")
    for n, (Cin, U, G) in enumerate(shapes):
        t, r64, r32 = E.composed_case(Cin, U, G)
        dev = {k: v.to(DEV).contiguous() for k, v in t.items()}
        PADF = 8                                                    # the forward operand with 8 spare columns: f_ld > 2 G
        wc_f = torch.full((Cin, 2 * G + PADF), FILL, device=DEV)
        wc_d = torch.full((2 * G + 1, Cin), FILL, device=DEV)       # one spare row
        bc = torch.full((2 * G + 3,), FILL, device=DEV)
        for dd in range(2):
            add(src=dev[f"wih{dd}"], dst_f=wc_f, dst_d=wc_d, Cout=G, Cin=Cin, KH=U, KW=1, kind=5, f_ld=2 * G + PADF, f_coff=dd * G, src2=dev["W1"],
                numel=G * Cin)
            add(src=dev[f"wih{dd}"], dst_f=bc, Cout=G, Cin=0, KH=U, KW=1, kind=6, f_coff=dd * G, src2=dev["b1"], src3=dev[f"bih{dd}"], numel=G)
            if n == 0 and dd == 0:                                    # a plain copy between the two directions
                src, dst = torch.randn(1000, generator=g).to(DEV), torch.zeros(1000, device=DEV)
                add(src=src, dst_f=dst, kind=2, KH=1, KW=1, numel=1000)
                extra.update(src=src, dst=dst)
            if n == 1 and dd == 0:                                    # a tiled kind-0 descriptor (Cout Cin >= 65536)
                w = torch.randn(256, 256, 3, 3, generator=g).to(DEV)
                wt_f, wt_d = torch.empty(9 * 256, 256, device=DEV), torch.empty(9 * 256, 256, device=DEV)
                assert lib.tpgsr_pack_blocks(0, 256, 256, 3, 3, w.numel()) == 64
                add(src=w, dst_f=wt_f, dst_d=wt_d, Cout=256, Cin=256, KH=3, KW=3, kind=0, f_ld=256, numel=w.numel())
                extra.update(w=w, wt_f=wt_f, wt_d=wt_d)
        keep.append(dev)
        want.append((Cin, U, G, PADF, wc_f, wc_d, bc, r64, r32))
    assert i == len(arr)
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    K.pack_program(table, len(arr), blk)
    torch.cuda.synchronize()
    src, dst, w, wt_f, wt_d = (extra[k] for k in ("src", "dst", "w", "wt_f", "wt_d"))
    assert torch.equal(dst, src)
    rf, rd = torch.empty_like(wt_f), torch.empty_like(wt_d)
    K.pack_conv_weight(w, 256, 256, 3, 3, rf, rd)
    torch.cuda.synchronize()
    assert torch.equal(wt_f, rf) and torch.equal(wt_d, rd)
    for Cin, U, G, PADF, wc_f, wc_d, bc, r64, r32 in want:
        wc_f, wc_d, bc = wc_f.cpu(), wc_d.cpu(), bc.cpu()
        assert (wc_f[:, 2 * G:] == FILL).all() and (wc_d[2 * G:] == FILL).all() and (bc[2 * G:] == FILL).all()
        bw, bb = E.arith_bound(r32["Wc"], r64["Wc"]), E.arith_bound(r32["bc"], r64["bc"])
        for name, got, ref, bound in (("dst_f", wc_f[:, :2 * G].T, r64["Wc"], bw), ("dst_d", wc_d[:2 * G], r64["Wc"], bw), ("bias", bc[:2 * G], r64["bc"], bb)):
            e = E.err(got, ref)
            WORST["pack 5/6"] = max(WORST.get("pack 5/6", 0.0), e / bound)
            print(f"pack kinds 5/6 ({Cin},{U},{G}) {name}: e {e:.2e}  bound {bound:.2e}  ratio {e / bound:.2f}")
            assert e <= bound, (Cin, U, G, name, e, bound)
        assert torch.equal(wc_f[:, :2 * G].T, wc_d[:2 * G])          # the two layouts hold the same numbers


def test_zz_report():
    for tag in sorted(WORST):
        print(f"engine GruLayer {tag}: worst e / bound {WORST[tag]:.2f}")
