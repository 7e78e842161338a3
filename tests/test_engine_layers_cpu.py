"""CPU: the one-layer engine harness of tests/engine_layer_common.py without a GPU.

In a child process with TPGSR_PLAN_DRYRUN=1 (tests/test_hd64_cpu.py's pattern) every case of tests/test_engine_gru_layer_gpu.py and
tests/test_engine_strip_fold_gpu.py is recorded into a K.Plan under every policy, the plan is handed to the native executor (entry points and
argument counts), and the recorded launch names are compared with the branch table those GPU files state (`expected_launches`): the one-launch
forward present or absent, tpgsr_bigru_bwd2 + tpgsr_gru_wgrad against tpgsr_bigru_bwd[_u] + 3 x tpgsr_conv_wgrad, tpgsr_compose_bwd_program
last -- so the GPU files provably cover the branches they name.  In-process: every float64 reference those files compare against is finite and
has every key, and the error models their bounds are derived from (e_ref32 of the `arith` rule, e_model of one-term arithmetic) are finite and
positive."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import engine_layer_common as E  # noqa: E402
import test_engine_gru_layer_gpu as TG  # noqa: E402
import test_gru_proj_gpu as TP  # noqa: E402

SCRIPT = r'''
import json, sys, torch
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
from tpgsr_amd import kernels as K
assert K.DRYRUN
import engine_layer_common as E
import test_engine_gru_layer_gpu as TG

def record(run):
    plan = K.Plan("one_layer")
    with K.recording(plan):
        run()
    assert len(plan)
    plan.run()                                       # the native executor checks entry point and argument count
    return [op[0] for op in plan.ops]

dev = torch.device("cpu")
out = {}
for policy in E.POLICIES:
    with E.conv_prec(policy):
        o = out[policy] = {}
        for c in E.gru_cases():
            o[c.id] = record(lambda: E.run_gru(c, dev))
        by_id = {c.id: c for c in E.gru_cases()}
        for cid, pol in TG.BRANCHES:
            if pol == policy:
                o[cid + "|dh2"] = record(lambda: E.run_gru(by_id[cid], dev, split_dh=True))
                o[cid + "|x2passes"] = record(lambda: E.run_gru(by_id[cid], dev, passes=2))
        for c in E.strip_cases():
            o[c.id] = record(lambda: E.run_strip(c, dev))
        for c in E.fold_cases():
            o[c.id] = record(lambda: E.run_fold(c, dev))
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


@pytest.mark.timeout(600)
def test_gru_layer_launch_sequences(recorded):
    for policy in E.POLICIES:
        got = recorded[policy]
        for c in E.gru_cases():
            assert got[c.id] == c.expected_launches(policy), (policy, c.id, got[c.id])
            assert got[c.id][-1] == "tpgsr_compose_bwd_program"
            assert ("tpgsr_bigru_proj_fwd" in got[c.id]) == c.fused_forward(policy)
            assert ("tpgsr_gru_wgrad" in got[c.id]) == ("tpgsr_bigru_bwd2" in got[c.id]) == c.fused_wgrad(policy)
            assert got[c.id].count("tpgsr_conv_wgrad") == (0 if c.fused_wgrad(policy) else 3)
    by_id = {c.id: c for c in E.gru_cases()}
    for cid, policy in TG.BRANCHES:
        assert recorded[policy][cid + "|dh2"] == by_id[cid].expected_launches(policy)
        assert recorded[policy][cid + "|x2passes"] == by_id[cid].expected_launches(policy, passes=2)


def test_the_branch_table_has_every_branch():
    """the cases reach: the one-launch forward on both axes and with both channel counts, the two-launch forward at 32 and at 64 units, both
    backward branches at 32 units and the 64-unit one -- and the cases the GPU file singles out sit on three different backward branches"""
    seen = set()
    for policy in E.POLICIES:
        for c in E.gru_cases():
            seen.add((c.fused_forward(policy), c.fused_wgrad(policy), c.Hd, c.axis, c.Cin if c.fused_forward(policy) else 0))
    for axis, cin in ((0, 64), (1, 64), (1, 96)):
        assert (True, True, 32, axis, cin) in seen
    assert {(False, True, 32), (False, False, 32), (False, False, 64)} <= {s[:3] for s in seen}
    assert not any(s[0] for s in seen if s[2] == 64)
    by_id = {c.id: c for c in E.gru_cases()}
    assert {(by_id[cid].fused_wgrad(p), by_id[cid].Hd) for cid, p in TG.BRANCHES} == {(True, 32), (False, 32), (False, 64)}
    assert {by_id[cid].fused_forward(p) for cid, p in TG.BRANCHES} == {True, False}


def test_strip_and_fold_launch_sequences(recorded):
    for policy in E.POLICIES:
        for c in E.strip_cases() + E.fold_cases():
            assert recorded[policy][c.id] == c.expected_launches(policy), (policy, c.id, recorded[policy][c.id])


def _finite(d, keys):
    assert set(d) == set(keys), (sorted(d), sorted(keys))
    for k, v in d.items():
        assert v.dtype == torch.float64 and bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0, k


def test_gru_references_are_finite_and_complete():
    for c in E.gru_cases():
        r = c.reference()
        _finite(r, ("h", "dx") + E.GRU_KEYS)
        assert tuple(r["h"].shape) == (c.P, 2 * c.Hd) and tuple(r["dx"].shape) == (c.P, c.Cin)
        for k, v in c.params.items():
            assert tuple(r[k].shape) == tuple(v.shape), k
        assert c.reference() is r                       # computed once, shared


def test_strip_and_fold_references_are_finite_and_complete():
    for c in E.strip_cases():
        r = c.reference()
        _finite(r, ("y", "dx", "dw"))
        assert tuple(r["dw"].shape) == (c.Cin, c.Cout, 3, 3) and float(r["dw"][:, :, 0].abs().max()) == 0 == float(r["dw"][:, :, 2].abs().max())
    for c in E.fold_cases():
        _finite(c.reference(), ("dx",))


def test_arith_error_models_are_finite_and_positive():
    """e_ref32 of every output of the direct kernel tests.  One departure from "positive": dbih = pre-fill + dbc is a single float32 addition,
    which can be exact, so e_ref32 may be 0 there and the bound is then the rule's floor, 4 * 2^-24, alone"""
    for shape in E.COMPOSE_SHAPES:
        _t, fill, r64, r32 = E.compose_case(*shape)
        _finite(r64, E.COMPOSE_OUT)
        assert set(fill) == set(E.COMPOSE_OUT) and all(float(v.abs().min()) > 0 for v in fill.values())
        for k in E.COMPOSE_OUT:
            e = E.err(r32[k], r64[k])
            assert math.isfinite(e) and e < 1e-5, (shape, k, e)
            assert e > 0 or k.startswith("dbih"), (shape, k)          # (dbih: one addition, float32 may be exact)
    for shape in E.COMPOSE_SHAPES[:3]:
        _t, r64, r32 = E.composed_case(*shape)
        _finite(r64, ("Wc", "bc"))
        for k in ("Wc", "bc"):
            e = E.err(r32[k], r64[k])
            assert math.isfinite(e) and 0 < e < 1e-5, (shape, k, e)


def test_fused_forward_matrix_references_and_bf16_model():
    """the fp64 recurrence of tests/test_gru_proj_gpu.py on every map of its matrix: finite, all four planes, and the one-term error model
    finite, positive and of bf16's size (2^-9 per operand)"""
    for N, H, W, axis in TP.MATRIX_MAPS:
        for loader in TP.MATRIX_LOADERS:
            h, gt, em_h, em_gt = TP.matrix_reference(N, H, W, axis, loader)
            assert tuple(h.shape) == (N * H * W, 64) and tuple(gt.shape) == (N * H * W, 256)
            assert bool(torch.isfinite(h).all()) and bool(torch.isfinite(gt).all())
            for e in [em_h] + em_gt:
                assert math.isfinite(e) and 0 < e < 1e-1, (N, H, W, axis, loader, e)
