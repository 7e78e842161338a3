"""CPU: the one-layer CRNN harness of tests/engine_crnn_layer_common.py without a GPU.

In a child process with TPGSR_PLAN_DRYRUN=1 (tests/test_engine_layers_cpu.py's pattern) every case of tests/test_engine_crnn_layers_gpu.py is
recorded into a K.Plan under every policy and run mode that file uses, the plan is handed to the native executor (entry points and argument
counts), and the recorded launch names are compared with the branch table (`expected_launches`): granule and counter forward, the per-step
pairs, five single weight gradients against tpgsr_conv_wgrad_batch (one launch for rnn1, two for rnn0), the reduce program, the BatchNorm
epilogue fused or not -- so the GPU file provably covers the branches it names.  The same child pins the batch limit: a CRNN forward with 65
images raises the named ValueError before a plan is recorded or a launch is made.  In-process: every float64 reference is finite, non-zero
and has every key with the parameter's shape, the ReLU margins hold, every e_ref32 and every error-model term is finite and positive (but
the terms of `EXACT`, which are zero: those gradients are column sums of the upstream gradient, no rounded operand enters them -- they can
widen no bound)."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import engine_crnn_layer_common as C  # noqa: E402
import test_engine_crnn_layers_gpu as TG  # noqa: E402
from test_functional_ops_gpu import MARGIN  # noqa: E402

SCRIPT = r'''
import json, sys, torch
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
from tpgsr_amd import kernels as K
assert K.DRYRUN
import engine_crnn_layer_common as C

def record(run):
    """an eager run, recorded: the native executor checks entry point and argument count of every launch"""
    plan = K.Plan("one_layer")
    with K.recording(plan):
        run()
    assert len(plan)
    plan.run()
    return [op[0] for op in plan.ops]

def recorded(case):
    """the harness's own recorded mode (it builds, closes and runs the plan itself)"""
    _got, names, eng = C.run_lstm(case, dev, mode="recorded")
    assert [op[0] for op in eng._plan.ops if op[1] is not None] == names
    assert {op[0] for op in eng._plan.ops if op[1] is None} == {"fork", "join"}      # the weight gradients sit on the side stream
    return names

class patched:
    def __init__(self, **kw):
        self.kw = kw
    def __enter__(self):
        self.prev = {k: getattr(K, k) for k in self.kw}
        for k, v in self.kw.items():
            setattr(K, k, v)
    def __exit__(self, *exc):
        for k, v in self.prev.items():
            setattr(K, k, v)

dev = torch.device("cpu")
out = {}
by_id = {c.id: c for c in C.lstm_cases()}
for policy in C.POLICIES:
    with C.conv_prec(policy):
        o = out[policy] = {}
        for c in C.lstm_cases():
            o[c.id] = record(lambda: C.run_lstm(c, dev))
        for cid, pol in C.RECORDED:
            if pol == policy:
                o[cid + "|recorded"] = recorded(by_id[cid])
        if policy == "f32":                      # (not a GPU test: the table's third weight-gradient form, deferred single launches)
            o["rnn1-2x5|recorded"] = recorded(by_id["rnn1-2x5"])
        for cid, pol in C.PER_STEP:
            if pol == policy:
                with patched(LSTM_SEQ=False, LSTM_SEQ_BWD=False):
                    o[cid + "|per_step"] = record(lambda: C.run_lstm(by_id[cid], dev))
        for cid, pol in C.GRANULE_OFF:
            if pol == policy:
                with patched(LSTM_GRANULE=False):
                    o[cid + "|granule_off"] = record(lambda: C.run_lstm(by_id[cid], dev))
        for cid, pol in C.TWO_PASSES:
            if pol == policy:
                o[cid + "|x2passes"] = record(lambda: C.run_lstm(by_id[cid], dev, passes=2))
        if policy in C.BN_POLICIES:
            for c in C.bn_cases():
                fused = []
                o[c.id] = record(lambda: fused.append(C.run_bn_lstm(c, dev)[2]))
                o[c.id + "|fused"] = fused[0]
        for c in C.conv0_cases():
            o[c.id] = record(lambda: C.run_conv0(c, dev)[1])

# the batch limit: 65 images raise before anything is bound, recorded or launched
from tpgsr_amd.model.crnn import crnn
net = crnn.CRNN(32, 1, 37, 256)
eng = net._engine()
with C.launch_log() as names:
    try:
        net(torch.zeros(65, 1, 32, 100))
        limit = "no error"
    except ValueError as e:
        limit = str(e)
out["limit"] = dict(message=limit, launches=names, plans=len(eng._plans))
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


BY_ID = {c.id: c for c in C.lstm_cases()}


@pytest.mark.timeout(600)
def test_lstm_layer_launch_sequences(recorded):
    seen = set()
    for policy in C.POLICIES:
        got = recorded[policy]
        for c in C.lstm_cases():
            assert got[c.id] == c.expected_launches(policy), (policy, c.id, got[c.id])
            assert ("tpgsr_lstm_seq_fwdg" in got[c.id]) == (c.T <= 31) and ("tpgsr_lstm_seq_fwd" in got[c.id]) == (c.T > 31)
            assert got[c.id].count("tpgsr_conv_wgrad") == got[c.id].count("tpgsr_wgrad_reduce") == 5
            assert got[c.id].count("tpgsr_pad_channels") == int(c.padded)
            seen |= set(got[c.id])
    for cid, policy in C.RECORDED:
        got = recorded[policy][cid + "|recorded"]
        assert got == BY_ID[cid].expected_launches(policy, "recorded"), (policy, cid, got)
        assert got.count("tpgsr_conv_wgrad_batch") == (2 if BY_ID[cid].loader == "relu" else 1) and "tpgsr_conv_wgrad" not in got
        seen |= set(got)
    got = recorded["f32"]["rnn1-2x5|recorded"]
    assert got == BY_ID["rnn1-2x5"].expected_launches("f32", "recorded") and got.count("tpgsr_conv_wgrad") == 5 and "tpgsr_wgrad_reduce" not in got
    for cid, policy in C.PER_STEP:
        got = recorded[policy][cid + "|per_step"]
        assert got == BY_ID[cid].expected_launches(policy, per_step=True), (policy, cid, got)
        assert not any(n.startswith("tpgsr_lstm_seq") for n in got)
        seen |= set(got)
    for cid, policy in C.GRANULE_OFF:
        got = recorded[policy][cid + "|granule_off"]
        assert got == BY_ID[cid].expected_launches(policy, granule=False) and "tpgsr_lstm_seq_fwd" in got, (policy, cid, got)
    for cid, policy in C.TWO_PASSES:
        assert recorded[policy][cid + "|x2passes"] == BY_ID[cid].expected_launches(policy, passes=2)
    # every branch the GPU file names was recorded at least once
    assert {"tpgsr_lstm_seq_fwdg", "tpgsr_lstm_seq_fwd", "tpgsr_lstm_seq_bwd", "tpgsr_lstm_rec_gemm", "tpgsr_lstm_step_fwd", "tpgsr_lstm_step_bwd",
            "tpgsr_conv_wgrad", "tpgsr_wgrad_reduce", "tpgsr_conv_wgrad_batch", "tpgsr_wgrad_reduce_program", "tpgsr_pad_channels"} <= seen


def test_batchnorm_and_conv0_launch_sequences(recorded):
    for policy in C.BN_POLICIES:
        for c in C.bn_cases():
            assert recorded[policy][c.id] == c.expected_launches(policy), (policy, c.id, recorded[policy][c.id])
            assert recorded[policy][c.id + "|fused"] == (policy == "x3") == ("tpgsr_bn_bwd_reduce" not in recorded[policy][c.id])
    for policy in C.POLICIES:
        for c in C.conv0_cases():
            assert recorded[policy][c.id] == c.expected_launches(policy), (policy, c.id, recorded[policy][c.id])
            assert "tpgsr_wgrad_reduce_program" in recorded[policy][c.id]        # (real = (9, 1, 1, 0): slab rows 9..11 skipped)


def test_batch_of_65_raises_before_anything_is_recorded(recorded):
    lim = recorded["limit"]
    assert "batch <= 64" in lim["message"] and "65" in lim["message"], lim
    assert lim["launches"] == [] and lim["plans"] == 0, lim
    from tpgsr_amd import engine_crnn
    assert engine_crnn.LstmLayer.MAX_BATCH == 64
    engine_crnn.LstmLayer.check_batch(64)
    with pytest.raises(ValueError, match="batch <= 64"):
        engine_crnn.LstmLayer.check_batch(65)
    from tpgsr_amd.model.crnn import crnn
    assert "64" in engine_crnn.LstmLayer.__doc__ and "64" in crnn.CRNN.__doc__


def test_the_branch_table_has_every_branch():
    """written from LstmLayer's code: both persistent forward kernels, the per-step pairs, single / batched (one and two launches) / deferred
    single weight gradients, the padded gradient"""
    t = {}
    for c in C.lstm_cases():
        for policy in C.POLICIES:
            t[(c.id, policy, "eager")] = c.expected_launches(policy)
    for cid, policy in C.RECORDED:
        t[(cid, policy, "recorded")] = BY_ID[cid].expected_launches(policy, "recorded")
    for cid, policy in C.PER_STEP:
        t[(cid, policy, "per step")] = BY_ID[cid].expected_launches(policy, per_step=True)
    for cid, policy in C.GRANULE_OFF:
        t[(cid, policy, "granule off")] = BY_ID[cid].expected_launches(policy, granule=False)
    names = set().union(*t.values())
    assert {"tpgsr_lstm_seq_fwdg", "tpgsr_lstm_seq_fwd", "tpgsr_lstm_seq_bwd", "tpgsr_lstm_rec_gemm", "tpgsr_lstm_step_fwd", "tpgsr_lstm_step_bwd",
            "tpgsr_conv_wgrad", "tpgsr_wgrad_reduce", "tpgsr_conv_wgrad_batch", "tpgsr_wgrad_reduce_program", "tpgsr_pad_channels"} <= names
    assert {v.count("tpgsr_conv_wgrad_batch") for k, v in t.items() if k[2] == "recorded"} == {1, 2}
    assert any("tpgsr_lstm_seq_fwd" in v for k, v in t.items() if k[0].endswith("1x33"))
    assert {BY_ID[cid].name for cid, _ in C.RECORDED} == {BY_ID[cid].name for cid, _ in C.PER_STEP} == {BY_ID[cid].name for cid, _ in C.TWO_PASSES} \
        == {"rnn0", "rnn1"}
    assert {(c.N, c.T) for c in C.lstm_cases()} == {(2, 5), (3, 26), (1, 33), (64, 2)}
    assert all(BY_ID[cid].T == 5 for cid, _ in C.PER_STEP)               # ten small launches per pass, not fifty


def _finite(d, keys):
    assert set(d) == set(keys), (sorted(d), sorted(keys))
    for k, v in d.items():
        assert v.dtype == torch.float64 and bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0, k


EXACT = ("embedding.bias", "db")     # plain column sums of the upstream gradient: no GEMM operand is rounded on the way, the model term is 0


def _positive(terms, keys):
    assert set(terms) == set(keys)
    for k, v in terms.items():
        assert math.isfinite(v) and (v < 1e-12 if k in EXACT else 0 < v < 1), (k, v)


def test_lstm_references_margins_and_error_models():
    for c in C.lstm_cases():
        r = c.reference()
        _finite(r, TG.LSTM_ALL)
        assert tuple(r["e"].shape) == (c.M, c.nOut) and tuple(r["out"].shape) == (c.M, 512) and tuple(r["dx"].shape) == (c.M, c.Cin)
        for k, v in c.params.items():
            assert tuple(r[k].shape) == tuple(v.shape), k
        assert c.reference() is r                       # computed once, shared
        z = c.pre_activation()
        if c.loader == "relu":
            assert z.abs().min().item() > MARGIN, (c.id, z.abs().min().item())
            assert 0.2 < (z > 0).double().mean().item() < 0.8      # both sides of the ReLU
        else:
            assert z is None
        for policy in ("x2", "bf16"):
            _positive(c.model_terms(policy), TG.LSTM_ALL)
        assert c.model_terms("x3") == {} == c.model_terms("f32")
        assert all(c.model_terms("x2")[k] < c.model_terms("bf16")[k] for k in TG.LSTM_ALL if k not in EXACT)
    assert set(TG.MODEL_KEYS) == {"x2", "bf16"} and all(set(v) <= set(TG.LSTM_ALL + ("ds", "y", "dw", "db", "dgray") + C.BN_KEYS) for v in TG.MODEL_KEYS.values())


def test_batchnorm_case_margin_and_reference():
    """the first seed of BN_SEEDS that keeps the float64 bn(s) 64 float32 errors away from the ReLU's kink: found, and which"""
    cases = C.bn_cases()
    assert [(c.M, (c.M + 63) // 64, c.M % 64) for c in cases] == [(10, 1, 10), (78, 2, 14)]
    for c in cases:
        print(f"{c.id}: seed {c.seed}, min |bn(s)| {c.margin:.2e}, float32 error of bn(s) {c.noise:.2e}")
        assert c.seed in C.BN_SEEDS and math.isfinite(c.margin) and c.noise > 0 and c.margin > C.BN_MARGIN_FACTOR * c.noise
        r = c.reference()
        _finite(r, ("e", "out", "ds") + C.BN_KEYS + C.LSTM_KEYS)
        assert tuple(r["ds"].shape) == (c.M, 512) and tuple(r["bn.weight"].shape) == (512,) == tuple(r["bn.bias"].shape)
        for policy in ("x2", "bf16"):
            _positive(c.model_terms(policy), r.keys())
    assert [c.seed for c in cases] == [c.seed for c in C.bn_cases()]          # deterministic


def test_conv0_references_and_direct_kernel_error_models():
    for c in C.conv0_cases():
        r = c.reference()
        _finite(r, ("y", "dw", "db", "dgray"))
        assert tuple(r["y"].shape) == (c.N * c.H * c.W, 64) and tuple(r["dw"].shape) == (64, 1, 3, 3) and tuple(r["db"].shape) == (64,)
        assert tuple(r["dgray"].shape) == (c.N, 1, c.H, c.W)
        for policy in ("x2", "bf16"):
            _positive(c.model_terms(policy), r.keys())
    for shape in C.COL_SHAPES:
        gray, want = C.im2col_case(*shape)
        assert tuple(want.shape) == (shape[0] * shape[1] * shape[2], 9) and float(want.abs().max()) > 0
        dcol, r64, r32 = C.col2im_case(*shape)
        assert float(dcol[:, 9:].abs().min()) > 100                          # the garbage in columns 9..11 would show
        assert bool(torch.isfinite(r64).all()) and float(r64.abs().max()) > 0
        e = C.err(r32, r64)
        # (1x1x1: one tap, the float32 adjoint is a copy and exact -- the bound is then the rule's floor, 4 * 2^-24, alone)
        assert math.isfinite(e) and e < 1e-6 and (e > 0 or shape == (1, 1, 1)), (shape, e)
        assert C.arith_bound(r32, r64) >= C.FLOOR > 0
    for shape in C.PAD_SHAPES:
        src, want = C.pad_case(*shape)
        assert tuple(want.shape) == (shape[0], shape[2]) and torch.equal(want[:, :shape[1]], src) and not bool(want[:, shape[1]:].any())
