"""CPU: the one host-side decision behind tpgsr_conv_fwd / tpgsr_conv_wgrad (csrc/conv_route.cpp).

tests/golden/conv_routes.json holds, for a deterministic sweep of argument blocks and for every block the engines' dry-run plans record
(tests/golden/make_golden_routes.py), the kernel and host-side launch parameters that the launchers' cascade chose in the commit BEFORE the
route function existed -- dumped there through a probe that called that commit's own predicates in the launchers' order -- and what its
planners answered.  Every case must still match, field for field; and the planners must say what the route says, for every case."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_routes as G  # noqa: E402


@pytest.fixture(scope="module")
def gold():
    from tpgsr_amd import build
    build.build()
    return G.load_golden()


@pytest.fixture(scope="module")
def fresh(gold):
    """the sweep and the recorded launches routed in a fresh process with none of the library's switches in its environment"""
    return G.run_emit(["sweep", "recorded"])


@pytest.fixture(scope="module")
def sweep(gold, fresh):
    cases = G.cases_of("sweep")
    assert fresh["sweep"]["args_crc"] == gold["sweep"]["args_crc"] and len(cases) == len(gold["sweep"]["rows"]), \
        "the sweep of make_golden_routes.py no longer builds the argument blocks the golden file was recorded for"
    return cases, fresh["sweep"]["rows"]


def _diff(cases, want, got, names):
    bad = []
    for (op, args, knobs), w, g in zip(cases, want, got):
        if w != g:
            f = names[op]
            bad.append(f"{op} {G.fields_of(args)} {knobs}: " + ", ".join(f"{n} {a} -> {b}" for n, a, b in zip(f, w, g) if a != b))
    return bad


def test_sweep_routes_match_the_recorded_cascade(gold, sweep):
    cases, rows = sweep
    names = {"fwd": gold["fwd_fields"], "wgrad": gold["wgrad_fields"]}
    bad = _diff(cases, gold["sweep"]["rows"], rows, names)
    assert not bad, f"{len(bad)} of {len(cases)} routes changed:\n" + "\n".join(bad[:20])


def test_sweep_reaches_every_kernel(sweep):
    from tpgsr_amd import _lib
    cases, rows = sweep
    fwd = {r[0] for (op, _, _), r in zip(cases, rows) if op == "fwd"}
    wg = {r[0] for (op, _, _), r in zip(cases, rows) if op == "wgrad"}
    assert fwd == set(range(len(_lib.CONV_KERNELS))), sorted(fwd)
    assert wg == set(range(len(_lib.WGRAD_KERNELS))), sorted(wg)
    ne = G.WG_FIELDS.index("ne")
    assert {r[ne] for (op, _, _), r in zip(cases, rows) if op == "wgrad"} == {0, 7, 9}      # both variants of the weight-gradient halo kernel
    nbw = G.FWD_FIELDS.index("nbw")
    assert {r[nbw] for (op, _, _), r in zip(cases, rows) if op == "fwd"} == {0, 1, 3}       # both panel shapes (K = 192 behind its switch)


def test_recorded_launches_match_the_recorded_cascade(gold, fresh):
    """every tpgsr_conv_fwd / tpgsr_conv_wgrad argument block of the TSRN_TL + CRNN cascade step at batch 48 and of one `_TL` backbone,
    under f32 / x3 / x2 / bf16 (pointers reduced to their alignment)"""
    blocks = gold["recorded_blocks"]
    assert len(blocks["order"]) > 300
    got = fresh["recorded"]
    assert got["args_crc"] == gold["recorded"]["args_crc"]
    bad = _diff(G.recorded_cases(blocks), gold["recorded"]["rows"], got["rows"], {"fwd": gold["fwd_fields"], "wgrad": gold["wgrad_fields"]})
    assert not bad, "\n".join(bad[:20])


def test_weight_gradient_halo_threshold_from_the_environment(gold, fresh):
    """TPGSR_XBF_WGRAD_HALO_MINWORK is read into ConvKnobs when the library loads: a fresh process with it at 0"""
    got = G.run_emit(["minwork0"], TPGSR_XBF_WGRAD_HALO_MINWORK="0")["minwork0"]
    assert got == gold["minwork0"]
    dflt = G.run_emit(["minwork0"])["minwork0"]
    assert any(row[0] == 3 for row in got["rows"][0::2]) and got["args_crc"] == dflt["args_crc"] and got["rows"] != dflt["rows"]      # the threshold moved something


def test_planners_say_what_the_route_says(sweep, gold, fresh):
    """tpgsr_conv_splitk_plan / tpgsr_conv_bn_row_tiles / tpgsr_conv_in2_scale_ok / tpgsr_wgrad_halo_plan sized a buffer or set an argument for
    the kernel the launcher is going to pick: for every case, their answers follow from the route of the launch they plan"""
    from tpgsr_amd import _lib
    HALO3, HALO, SPLITK = (_lib.CONV_KERNELS.index(k) for k in ("xbf_halo3", "xbf_halo", "xbf_splitk"))
    WG_HALO = _lib.WGRAD_KERNELS.index("xbf_halo")
    cases, rows = sweep
    cases = cases + G.recorded_cases(gold["recorded_blocks"])
    rows = rows + fresh["recorded"]["rows"]
    F, W = {n: i for i, n in enumerate(gold["fwd_fields"])}, {n: i for i, n in enumerate(gold["wgrad_fields"])}
    for (op, args, knobs), row in zip(cases, rows):
        if op == "fwd":
            assert row[F["splitk_plan"]] == row[F["sk_plan"]]
            if row[F["splitk_plan"]] > 1:          # the proposal, taken: the launcher runs split-K with exactly that many splits
                M = args.N * args.OH * args.OW
                assert row[F["sk_bytes"]] == row[F["splitk_plan"]] * ((M + 63) // 64) * ((args.Cout + 63) // 64) * 256 * 16 * 4
                assert (row[F["sk_taken_kernel"]], row[F["sk_taken_splits"]]) == (SPLITK, row[F["splitk_plan"]])
            else:
                assert row[F["splitk_plan"]] == 0 and row[F["sk_bytes"]] == 0
            if not args.sk_splits > 1 and not args.in2_scale:
                assert row[F["bn_row_tiles"]] == (3 if row[F["kernel"]] == HALO3 else 1)
            if args.in2_scale and not args.sk_splits > 1:
                assert row[F["in2_scale_ok"]] == (1 if row[F["kernel"]] == HALO3 else 0)
            if row[F["kernel"]] == HALO:
                assert row[F["lcap"]] == row[F["halo_capacity"]]
        else:
            # the plan proposes the halo kernel's split count; a launch that follows it (zsplits, dy_bf, a loader the kernel has) lands there
            if row[W["kernel"]] == WG_HALO:
                assert row[W["halo_plan"]] == 1 and row[W["Z"]] == args.zsplits
            follows = args.dy_bf and args.zsplits > 0 and (args.c.Cin & 3) == 0 and (row[W["vecY"]] or args.dy_ps) and row[W["ld"]] in (0, 1, 2, 3, 4, 5, 7)
            if row[W["halo_plan"]] and follows:
                assert row[W["kernel"]] == WG_HALO
            if not args.zsplits:
                assert row[W["Z"]] == row[W["wgrad_splits"]]


def test_back_channel_exports_are_gone():
    """one translation unit no longer asks another through the C ABI; the route itself is exported instead"""
    from tpgsr_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("tpgsr_conv_halo3_would_take", "tpgsr_conv_panel_would_take", "tpgsr_loader_bits", "tpgsr_wgrad_plan_host",
                 "tpgsr_conv_fwd_xbf_launch", "tpgsr_conv_wgrad_xbf_launch", "tpgsr_conv_wgrad_halo_launch", "tpgsr_conv_panel_xbf_launch",
                 "tpgsr_halo_set_ne9"):
        assert not hasattr(lib, name), name
    for name in ("tpgsr_conv_route", "tpgsr_conv_wgrad_route"):
        assert hasattr(lib, name), name


def test_kernels_conv_route():
    from tpgsr_amd import _lib, kernels as K
    a = G.conv_args(48, 16, 64, 64, 64, 3, 3, 1, 1, terms=2)
    name, r = K.conv_route(a)
    assert name == "xbf_halo3" and r.lds_bytes == 161792 and r.lcap > 0
    lib = _lib.load()
    lib.tpgsr_halo3_set_enabled(0)
    try:
        assert K.conv_route(a)[0] == "xbf_halo"
    finally:
        lib.tpgsr_halo3_set_enabled(1)
    assert K.conv_route(G.conv_args(48, 16, 64, 64, 64, 3, 3, 1, 1))[0] == "f32_wstat"
    name, r = K.conv_route(G.wgrad_args(G.conv_args(48, 16, 64, 64, 192, 1, 1, terms=2)))
    assert name == "xbf_tile" and r.vecY == 1 and r.Z * r.MB >= 48 * 16 * 64
    with pytest.raises(ValueError):          # the exported route refuses a geometry it would divide by, as the launchers do
        K.conv_route(_lib.ConvArgs())
    assert lib.tpgsr_conv_wgrad_route(C.byref(_lib.WgradArgs()), C.byref(_lib.WgradRoute())) == -1


def test_route_alone_under_the_host_sanitizers(tmp_path):
    """tools/conv_route_check.cpp: conv_route.cpp linked alone (no HIP, no Python) over the sweep's geometry, under ASan + UBSan"""
    import shutil
    import subprocess
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "conv_route_check")
    subprocess.run([cxx, "-std=c++20", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "conv_route_check.cpp"), os.path.join(ROOT, "tpgsr_amd", "csrc", "conv_route.cpp"), "-o", exe],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
