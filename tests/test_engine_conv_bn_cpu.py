"""CPU: the section harness of tests/engine_conv_bn_common.py without a GPU.

In a child process with TPGSR_PLAN_DRYRUN=1 every case of tests/test_engine_conv_bn_gpu.py is run under every policy and both run modes
(argument lists checked against the C ABI, the recorded plan handed to the native executor, nothing computed) and its launch names are
compared with the case's branch table; the same child records the real TSRNEngine plans of TSRN(STN=True, mask=True) and TSRN_TL(STN=True,
mask=True) at the default widths, and each section's forward / backward launch sequence must occur, in order, inside the engine's
tsrn_fwd_pre + tsrn_fwd / tsrn_bwd plan (the weight-gradient stream's launches, which the engine holds back behind one fork per side batch,
among themselves; the pack and slab-reduce programs separately) -- a section cannot drift into a private copy of the launch order.  The
seeded trunk variant under a split policy (bn2's backward pass with its own statistics launch) is held against a plan recorded with
`leaf_early` on, the one form of the engine that records it: contiguously, from that plan's first tpgsr_bn_bwd_reduce.
In process: every case has a finite float64 reference for every key, a finite float32-CPU error, inputs under 8 MiB and a positive bound; the
committed STN seed is the first of its list with no ReLU / max-pool decision inside the margin, in float64 and float32 alike (block1's seed
likewise, for the PReLU's kink); and the defects the issue names, applied to the reference, exceed a bound tenfold."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import engine_conv_bn_common as C  # noqa: E402
import test_engine_conv_bn_gpu as TG  # noqa: E402

SCRIPT = r'''
import json, sys, torch
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
from tpgsr_amd import kernels as K
assert K.DRYRUN
import engine_conv_bn_common as C
from tpgsr_amd.model import tsrn
dev = torch.device("cpu")
out = {}
cases = C.all_cases()
nets = {"tsrn": tsrn.TSRN(STN=True, mask=True).train(), "tsrn_tl": tsrn.TSRN_TL(STN=True, mask=True).train()}
for policy in C.POLICIES:
    o = out[policy] = {}
    with C.conv_prec(policy):
        for c in cases:
            for mode in C.MODES:
                _got, names, seen = C.run_case(c, dev, mode)
                o[c.id + "|" + mode] = names
                o[c.id + "|" + mode + "|seen"] = {k: v for k, v in seen.items() if k != "tail"}
        o["eval"] = C.run_bn_eval(cases[0], dev)[1]
        for tag, net in nets.items():
            eng = net._engine()
            eng.bind(dev)
            pl = eng.plans(2, 16, 64, True)
            for k in ("pre", "fwd", "bwd"):
                pl[k].run()                              # the native executor: entry point and argument count of every launch
            o[tag] = {k: [op[0] for op in pl[k].ops if op[1] is not None] for k in ("pre", "fwd", "bwd")}
        # block 0's convolution gradients on the leaf stream (TPGSR_LEAF_EARLY=1): there bn2's backward pass keeps its own statistics launch
        net = tsrn.TSRN(STN=True, mask=True).train()
        eng = net._engine()
        eng.leaf_early = True
        eng.bind(dev)
        pl = eng.plans(2, 16, 64, True)
        pl["bwd"].run()
        o["tsrn_leaf_early"] = {k: [op[0] for op in pl[k].ops if op[1] is not None] for k in ("pre", "fwd", "bwd")}
print("RESULT " + json.dumps(out))
'''


@pytest.fixture(scope="module")
def recorded():
    env = dict(os.environ, TPGSR_PLAN_DRYRUN="1")
    for k in [k for k in env if k.startswith("TPGSR_") and k != "TPGSR_PLAN_DRYRUN"]:
        del env[k]                                      # the recorded branches are the default ones
    r = subprocess.run([sys.executable, "-c", SCRIPT % dict(root=ROOT, tests=os.path.join(ROOT, "tests"))], capture_output=True, text=True, env=env,
                       timeout=550)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


CASES = TG.CASES


@pytest.mark.timeout(600)
def test_section_launch_sequences(recorded):
    seen_names = set()
    for policy in C.POLICIES:
        split = bool(C.TERMS[policy])
        got = recorded[policy]
        for c in CASES:
            for mode in C.MODES:
                names = got[f"{c.id}|{mode}"]
                assert names == c.expected_launches(policy, mode), (policy, c.id, mode, names)
                assert names[:len(C._pack_names(policy))] == C._pack_names(policy)
                seen_names |= set(names)
                seen = got[f"{c.id}|{mode}|seen"]
                if isinstance(c, C.TrunkCase):
                    assert tuple(seen["fused"]) == c.fused(policy) and names.count("tpgsr_bn_bwd_reduce") == 2 - sum(seen["fused"])
                    assert names.count("tpgsr_bn_finalize") == (2 if mode == "eager" else 4)
                if isinstance(c, C.UpCase):
                    assert seen["mish_epilogue"] == split == seen["fused"] and ("tpgsr_act_bwd" in names) == (not split)
        assert got["eval"] == ["tpgsr_bn_finalize"]
    assert {"tpgsr_bn_bwd_reduce", "tpgsr_act_bwd", "tpgsr_tail_bwd", "tpgsr_tail_shiftsum_tanh", "tpgsr_prelu_fwd", "tpgsr_prelu_bwd",
            "tpgsr_reduce_partials", "tpgsr_affine_act_pool", "tpgsr_affine_act_pool_bwd", "tpgsr_wgrad_reduce", "tpgsr_wgrad_reduce_program",
            "tpgsr_conv_wgrad", "tpgsr_affine_act", "tpgsr_bn_finalize", "tpgsr_bn_bwd_finalize", "tpgsr_bn_bwd_apply"} <= seen_names


def _split(names):
    return [n for n in names if n not in C.SIDE_NAMES], [n for n in names if n in C.SIDE_NAMES and n != "tpgsr_wgrad_reduce_program"]


@pytest.mark.timeout(600)
def test_sections_follow_the_engine_plans(recorded):
    """each section's launch names occur, in order, in the real engine's plans -- TSRN and TSRN_TL, every policy"""
    for policy in C.POLICIES:
        pack = C._pack_names(policy)
        for tag in ("tsrn", "tsrn_tl"):
            pl = recorded[policy][tag]
            fwd_plan, (bwd_main, bwd_side) = pl["pre"] + pl["fwd"], _split(pl["bwd"])
            assert pl["pre"][:len(pack)] == pack and not set(pack) & set(pl["pre"][len(pack):] + pl["fwd"] + pl["bwd"]), (policy, tag)
            assert 1 <= pl["bwd"].count("tpgsr_wgrad_reduce_program") <= 2 and "tpgsr_wgrad_reduce" not in pl["bwd"]
            for c in CASES:
                if isinstance(c, C.TrunkCase) and c.variant == "seeded" and C.TERMS[policy]:
                    continue      # bn2's unfused backward under a split policy: the engine's `leaf_early` form of block 0, checked below
                s = c.sections(policy, "recorded", fwd_passes=1) if isinstance(c, C.TrunkCase) else c.sections(policy, "recorded")
                assert C.is_subsequence(s["fwd"], fwd_plan), (policy, tag, c.id, "forward")
                main, side = _split(s["bwd"])
                assert C.is_subsequence(main, bwd_main), (policy, tag, c.id, "backward", main)
                assert C.is_subsequence(side, bwd_side), (policy, tag, c.id, "backward, weight-gradient stream", side)
                names = recorded[policy][f"{c.id}|recorded"]
                assert names[:len(pack)] == pack and names[-1] == "tpgsr_wgrad_reduce_program"
        if C.TERMS[policy]:
            early = recorded[policy]["tsrn_leaf_early"]
            e_main, e_side = _split(early["bwd"])
            default_main = _split(recorded[policy]["tsrn"]["bwd"])[0]
            assert e_main.count("tpgsr_bn_bwd_reduce") == default_main.count("tpgsr_bn_bwd_reduce") + 1       # block 0's bn2, and only it
            for c in CASES:
                if isinstance(c, C.TrunkCase) and c.variant == "seeded":
                    s = c.sections(policy, "recorded", fwd_passes=1)
                    main, side = _split(s["bwd"])
                    # (anchored at the first statistics launch of the plan -- block 0's bn2; the STN head's come after it)
                    at = e_main.index("tpgsr_bn_bwd_reduce")
                    assert e_main[at:at + len(main)] == main, (policy, c.id, e_main[at:at + len(main)], main)
                    assert C.is_subsequence(s["fwd"], early["pre"] + early["fwd"]) and C.is_subsequence(side, e_side), (policy, c.id)
    assert not C.is_subsequence(["tpgsr_bn_finalize", "tpgsr_tail_bwd", "tpgsr_bn_finalize"], recorded["x3"]["tsrn"]["bwd"])      # (the helper can fail)


def test_every_case_is_well_posed():
    assert [(c.N, c.H, c.W) for c in CASES if isinstance(c, C.TrunkCase) and c.C == 64] == [m for m in C.TRUNK_MAPS for _v in C.TRUNK_VARIANTS]
    assert [c.M % 64 for c in CASES if isinstance(c, C.TrunkCase)] == [0, 0, 0, 0, 41, 41, 41]
    stn = CASES[-1]
    assert stn.Ms == [5120, 1280, 320, 80, 20, 10, 5] and sum(m < 64 for m in stn.Ms) == 3
    for c in CASES:
        assert c.input_bytes() < C.SIZE_LIMIT, c.id
        r64, r32 = c.reference(), c.ref32()
        assert c.reference() is r64 and set(c.keys) <= set(r64) and set(c.zero_bias) <= set(c.keys) and set(c.values) <= set(c.keys), c.id
        assert {k for k in c.params if not k.startswith("proj.")} <= set(c.keys), c.id          # every parameter gradient is compared
        for key in c.keys:
            v = r64[key]
            assert v.dtype == torch.float64 and r32[key].dtype == torch.float32 and bool(torch.isfinite(v).all()), (c.id, key)
            assert float(v.abs().max()) > 0 or key in c.zero_bias, (c.id, key)
            e32 = c.e_ref32(key)
            assert math.isfinite(e32) and e32 < 1e-3, (c.id, key, e32)
            for policy in C.POLICIES:
                b = TG.bound(c, key, policy)
                assert math.isfinite(b) and b >= C.FLOOR and (c.g[key] > 0 or key in TG.model_keys(c, policy) or b == 4 * e32 + C.FLOOR), (c.id, key)
        for key, den in c.zero_bias.items():      # analytically zero: tiny against the summed column's |dy|
            assert float(torch.where(r64[den] > 0, r64[key].abs() / r64[den], r64[key].abs()).max()) < 1e-12, (c.id, key)


def test_stn_and_block1_seeds_keep_the_margins():
    """no ReLU pre-activation within 8 * 2^-24 * (|scale y| + |shift|) of zero and no pool window whose two largest entries lie within that
    distance of each other, on the float64 reference and on its float32 twin: zero decisions of 1e-4 allowed, for the first such seed"""
    assert C.first_stn_seed() == C.STN_SEED in C.STN_SEEDS
    stn = CASES[-1]
    assert stn.seed == C.STN_SEED
    for dtype in (torch.float64, torch.float32):
        d = stn.decisions(dtype)
        assert len(d) == 7 and [n for _r, _q, n in d] == [m * co for m, co in zip(stn.Ms, [co for _ci, co in C.STN_CH] + [512])]
        print(dtype, d)
        assert all((r + q) / n <= 1e-4 for r, q, n in d) and all(r == 0 and q == 0 for r, q, _n in d)
    a = stn.reference()
    assert 0.2 < float((a["ctrl"] != 0).double().mean())
    for c in CASES:
        if isinstance(c, C.Block1Case):
            print(c.id, "seed", c.seed, "near the kink", c.near)
            assert c.seed in C.B1_SEEDS and c.near == (0, 0)
            c1 = c.reference()["c1"]
            assert 0.05 < float((c1 < 0).double().mean()) < 0.95      # both sides of the PReLU


def _exceeds(case, mutated, keys, factor=10.0):
    """the worst e / bound of the mutated tensors over `keys`, per policy: >= factor (tenfold) under x3, x2 and f32.  Under bf16 only `above the
    bound` is asserted: the per-GEMM limit there is 2e-2, so g of them already put a bound at 0.04 .. 0.3 of max |ref| and tenfold of that is more
    than a wrong tensor of the right magnitude can differ by -- and the STN head's bf16 gradient bounds exceed 1 altogether (the GPU file's
    docstring), which is why `fc1 taps swapped` shows there only through ctrl (6 x)"""
    out = {}
    for policy in C.POLICIES:
        out[policy] = max(case.key_err(k, mutated[k]) / TG.bound(case, k, policy) for k in keys)
        assert out[policy] >= (factor if policy != "bf16" else 1.0), (case.id, policy, out[policy])
    return out


def test_the_named_defects_would_be_caught():
    by = {c.id: c for c in CASES}
    stn, ragged, up = CASES[-1], by["trunk-C64-3x5x7-seeded"], by["up-C64-1x5x7"]
    r = {}
    m = stn._autograd(torch.float64, 0, mutate="fc1_taps")
    r["fc1 taps swapped"] = _exceeds(stn, m, ["ctrl", C.FC1 + ".weight", C.CP[5] + ".0.weight"])
    m = stn._autograd(torch.float64, 0, mutate="fc2_scale")
    r["fc2's 0.1 dropped from the gradient"] = _exceeds(stn, m, [C.FC2 + ".weight"])
    for c in (ragged, by["trunk-C64-2x16x64-proj"]):
        m = c._autograd(torch.float64, 0, mutate="rm_without_bias")
        r["conv bias left out of running_mean " + c.id] = _exceeds(c, m, ["bn1.running_mean@1", "bn1.running_mean@2"])
    m = ragged._autograd(torch.float64, 0, mutate="stat_tail_dropped")
    r["last M % 64 rows dropped from the BatchNorm sums"] = _exceeds(ragged, m, ["bn1.save_mean", "bn1.save_rstd"])
    for c in (up, by["up-C64-2x16x64"]):
        m = c._autograd(torch.float64, 0, mutate="ps_phase")
        r["pixel-shuffle phase permuted " + c.id] = _exceeds(c, m, ["sr", "tail.weight", "up.weight"])
    for k, v in r.items():
        print(k, {p: f"{x:.3g}" for p, x in v.items()})


def test_every_model_key_is_needed():
    """a key carries the error-model term only where the float64 section on k-term operands ALONE (no margin factor) leaves the rule's bound in
    some case, or where the GPU left it by a recorded factor and the model alone is of the same order (over half the bound)"""
    entries = set()
    for policy, per_class in TG.MODEL_KEYS.items():
        assert policy in ("x2", "bf16")
        for cls, keys in per_class.items():
            cases = [c for c in CASES if type(c).__name__ == cls]
            assert cases and all(k in c.keys for c in cases for k in keys), (policy, cls)
            for k in keys:
                entries.add((policy, cls, k))
                alone = max(c.model_term(k, policy) / C.MODEL_MARGIN / c.bound(k, policy) for c in cases)
                miss = TG.RECORDED_MISS.get((policy, cls, k))
                print(f"{policy} {cls} {k}: model e / rule's bound {alone:.2f}" + (f", recorded GPU miss {miss}" if miss else ""))
                assert (alone > 1) != (miss is not None), (policy, cls, k, alone, miss)
                assert miss is None or (miss > 1 and alone > 0.5), (policy, cls, k, alone, miss)
    assert set(TG.RECORDED_MISS) <= entries
    for c in CASES:
        assert all(c.model_term(k, p) == 0.0 for k in c.keys[:2] for p in ("x3", "f32"))
