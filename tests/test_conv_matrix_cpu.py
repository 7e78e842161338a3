"""CPU: the case table of tests/conv_matrix_common.py is complete, routed where it says, and well posed.

* route per case: tpgsr_conv_route / tpgsr_conv_wgrad_route on the case's argument block (fake aligned pointers, built by the same
  `block` the GPU test launches) returns exactly the case's kernel, loader variant and terms, and the host parameters it pins (nbw, ne,
  splits, Z, vecY, bn_row_tiles);
* completeness from the route: for one geometry per (kernel, shape class), every ld 0 .. 63 x T 0 .. 3 is probed; the set the route gives
  to the kernel equals the set of cases the table has for it -- a new instantiation without a case fails here, and so does a case for a
  variant that no longer exists (the batch kernel's set is read through tpgsr_conv_wgrad_batch_prepare);
* recorded classes: every (kernel, terms, loader, epilogue class) of the engines' recorded launches (tests/golden/conv_routes.json)
  maps onto a case; split-K and the halo weight gradient, which a dry run cannot see, are there for every T;
* every epilogue class of a kernel's list appears on that kernel for every T;
* well-posedness: sizes, ReLU margins, finite references with every key, and the float32-CPU reference inside every bound."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import conv_matrix_common as M  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def lib():
    from tpgsr_amd import build, _lib
    build.build()
    return _lib.load()


IDS = [f"{op}-{k}-T{T}" for op, k, T in M.GROUPS]


def test_matrix_size():
    n = {}
    for c in M.CASES:
        n[(c.op, c.kernel)] = n.get((c.op, c.kernel), 0) + 1
    print(f"{len(M.CASES)} cases:", ", ".join(f"{op} {k} {v}" for (op, k), v in sorted(n.items())))
    combos = {(c.op, c.kernel, c.ld, c.T, c.cls) for c in M.CASES}
    assert len(combos) >= 245 and len(M.GROUPS) == 30, (len(combos), len(M.GROUPS))


@pytest.mark.parametrize("grp", M.GROUPS, ids=IDS)
def test_route_per_case(grp):
    for c in M.group(*grp):
        M.assert_route(c)
        if c.mate is not None:
            M.assert_route(c.mate)
        blk = M.block(c, M.fake_ptrs())
        assert (blk.c.terms if c.op != "fwd" else blk.terms) == c.T, c.id


def _accepted(op, kernel, cls, knobs, geom):
    """{(ld, T)} the route sends to `kernel` on one geometry, everything else equal"""
    got = set()
    for ld in range(64):
        for T in range(4):
            c = M.MCase(op, kernel, T, ld, cls, geom, ("z",) if op == "wgrad" and kernel == "xbf_halo" else (), knobs, 0)
            name, r = M.route_of(c)
            if name == kernel:
                assert r.ld == ld
                got.add((ld, T))
    return got


@pytest.mark.parametrize("key", [k for k in M.KERNELS if k[0] != "batch"], ids=lambda k: "-".join(k))
def test_completeness_from_the_route(key):
    op, kernel = key
    lds, terms, classes, _ = M.KERNELS[key]
    for cls, (knobs, geoms) in classes.items():
        geom = next(g for g in geoms if g[4] % 4 == 0)
        have = {(c.ld, c.T) for c in M.CASES if (c.op, c.kernel, c.cls) == (op, kernel, cls)}
        got = _accepted(op, kernel, cls, knobs, geom)
        assert got == have, f"{op} {kernel} {cls}: instantiated without a case {sorted(got - have)}, cases without an instantiation {sorted(have - got)}"
        assert have == {(ld, T) for ld in lds for T in terms}


def test_completeness_of_the_batch_kernel(lib):
    from tpgsr_amd import _lib as L
    lds, terms, classes, _ = M.KERNELS[("batch", "batch")]
    geom = classes[""][1][0]
    got = set()
    for ld in range(64):
        for T in range(4):
            c = M.MCase("batch", "batch", T, ld, "", geom, (), {}, 0)
            if lib.tpgsr_conv_wgrad_batch_prepare(C.byref(M.block(c, M.fake_ptrs())), C.byref(L.WgradBatchItem())) >= 0:
                got.add((ld, T))
    have = {(c.ld, c.T) for c in M.CASES if c.op == "batch"}
    assert got == have == {(ld, T) for ld in lds for T in terms}, (sorted(got - have), sorted(have - got))


def test_run_time_loader_kernels():
    """the scalar kernels branch on the loader at run time: the route gives them every ld, the table has every loader bit and Cin 1 and 3"""
    for op, kernel in M.RUNTIME_LOADER:
        cases = [c for c in M.CASES if (c.op, c.kernel) == (op, kernel)]
        assert _accepted(op, kernel, "", {}, (3, 5, 13, 3, 40, 3, 3, 1, 1)) == {(ld, T) for ld in range(64) for T in range(4)}
        bits = 0
        for c in cases:
            bits |= c.ld
        assert bits & 31 == 31 and {1, 3} <= {c.Cin for c in cases}, (op, bits)


def _classes_of(op, st):
    a = st if op == "fwd" else st.c
    e = []
    if op == "fwd":
        if a.bias:
            e.append("bias")
        if a.out_act:
            e.append({1: "relu", 3: "tanh"}[a.out_act])
        if a.out_ps:
            e.append("ps")
        if a.bnb_y:
            e.append(f"bnb{a.bnb_act}" if a.bn_partial else "dzonly")
            if a.bnb_store_dz and a.bn_partial:
                e.append("dz")
        elif a.bn_partial:
            e.append("bn")
        if a.bn_row_tiles == 3:
            e.append("rt3")
        if a.out_ld != a.Cout or a.out_coff:
            e.append("outwin")
        if a.wt_ld or a.wt_coff:
            e.append("wtwin")
    else:
        if st.dbpart:
            e.append("db")
        if st.dy_ld != a.Cout or st.dy_coff:
            e.append("dywin")
        if st.dy_ps:
            e.append("dyps")
        if st.zsplits:
            e.append("z")
    if (a.in_ld != (a.cin_a if a.in_b else a.Cin) and not a.in_ps) or a.in_coff:
        e.append("inwin")
    if a.stride_w > 1:
        e.append("stride")
    if a.in_dil_w > 1:
        e.append("dil")
    return e


def test_recorded_classes_map_onto_cases():
    import make_golden_routes as G
    from tpgsr_amd import kernels as K
    have, plain = set(), set()
    for c in M.CASES:
        kernel = c.kernel
        plain.add((c.op, kernel, c.T, c.ld))
        for f in c.flags:
            have.add((c.op, kernel, c.T, c.ld, f))
    missing, seen = set(), set()
    for op, st, _ in G.recorded_cases(G.load_golden()["recorded_blocks"]):
        name, r = K.conv_route(st)
        T = (st if op == "fwd" else st.c).terms if name.startswith("xbf") else 0
        seen.add((op, name, T))
        if (op, name, T, r.ld) not in plain:
            missing.add((op, name, T, r.ld))
        for f in _classes_of(op, st):
            if (op, name, T, r.ld, f) not in have:
                missing.add((op, name, T, r.ld, f))
    assert not missing, sorted(missing)
    assert len(seen) > 15
    # what the dry run cannot see (K.conv_fwd / K.wgrad_splits skip both planners under DRYRUN): present for every T all the same
    for T in (1, 2, 3):
        assert M.group("fwd", "xbf_splitk", T) and M.group("wgrad", "xbf_halo", T), T
        assert ("fwd", "xbf_splitk", T) not in seen and ("wgrad", "xbf_halo", T) not in seen


def test_every_epilogue_class_on_every_kernel_for_every_term_count():
    for (op, kernel), (lds, terms, classes, epis) in M.KERNELS.items():
        want = set()
        for cls in classes:
            for e in M.CLASS_EPI.get((op, kernel, cls), epis):
                want.update(e)
        for T in terms:
            got = set()
            for c in M.group(op, kernel, T):
                got.update(c.flags)
            assert want <= got, (op, kernel, T, sorted(want - got))


def test_edges_of_every_kernel():
    """ragged M, ragged Cout, a tile spanning rows and images, N = 1 -- on every kernel whose geometry allows them"""
    for (op, kernel) in list(M.KERNELS) + list(M.RUNTIME_LOADER):
        cases = [c for c in M.CASES if (c.op, c.kernel) == (op, kernel)]
        if kernel != "f32_wstat":                 # (64 x 64 channels on 64-wide rows: nothing ragged by construction)
            assert any(c.M % 64 for c in cases) and any(c.Cout % 64 for c in cases), (op, kernel)
            assert any(c.OW % 64 and (c.OH * c.OW) % 64 and c.N > 1 for c in cases), (op, kernel)
        if kernel != "batch":
            assert any(c.N == 1 for c in cases) or kernel == "xbf_halo3", (op, kernel)


@pytest.mark.parametrize("grp", M.GROUPS, ids=IDS)
def test_well_posed(grp):
    for c in M.group(*grp):
        M.check_well_posed(c)
        if c.mate is not None:
            M.check_well_posed(c.mate)
        _, _, _, d_loader, d_ulp = M.references(c)
        print(f"{c.id}: seed {c.seed}  d_loader {max(d_loader.values()):.2e}  d_ulp {max(d_ulp.values()):.2e}")
