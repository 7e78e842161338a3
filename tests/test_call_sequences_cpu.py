"""CPU (TPGSR_PLAN_DRYRUN=1): the host side of the mixed call sequences of tests/test_call_sequences_gpu.py -- one long-lived module, train
step or cascade serving batch sizes 4, 6, 1, 4 with evaluation in between (tests/call_sequence_common.py).  Nothing is computed in a dry
run, so what is compared is what a call LAUNCHES: the trace of call k on the long-lived object (every launch outside a recording with its
scalar arguments, every replayed plan with the names, streams and scalar arguments of its ops) equals the trace of that call on a fresh
twin.  One difference is by design and filtered out: an eval-mode engine packs its operands only when the parameters changed since the last
pack (engine._EngineBase.pack_if_stale), so the long-lived object skips the `tsrn_pack` / `crnn_pack` plan a fresh one runs.

Also here, because it needs no device: the plan cache holds one entry per key served; a plan recorded before the shared scratch was
regrown keeps its old scratch tensors alive (`Plan.keep`); a train step keeps the static buffers of every shape it served (a captured
graph holds their addresses) while `_static` stays the set of the current shape; the functional engines refuse a backward pass whose slot
was overwritten at another batch size with the RuntimeError the TSRN engine gives."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

SCRIPT = r'''
import gc, json, sys, weakref, torch
sys.path[:0] = [%(root)r, %(tests)r]
from tpgsr_amd import kernels as K
assert K.DRYRUN
import call_sequence_common as C
DEV = "cpu"
lines = C.install_trace()
SKIPPED_WHEN_PACKED = ("plan tsrn_pack ", "plan crnn_pack ")

def traced(obj, op):
    del lines[:]
    C.run_call(obj, op, DEV)
    return [l for l in lines if not l.startswith(SKIPPED_WHEN_PACKED)]

def sequence(builder, seq):
    A, calls = builder(), []
    for op in seq:
        snap = C.snapshot(A)
        ta = traced(A, op)
        tb = traced(C.fresh_twin(snap, builder), op)
        first = next((i for i, (a, b) in enumerate(zip(ta, tb)) if a != b), None)
        calls.append(dict(op=list(op), lines=len(ta), twin_lines=len(tb), plans=sum(l.startswith("plan ") for l in ta),
                          first_difference=None if first is None else [first, ta[first], tb[first]]))
    return A, calls

def n_plans(obj):
    return [len(m._engine()._plans) for m in C.modules_of(obj)]

res = dict(eval={}, step={}, cascade={})
for name in ("tsrn", "tsrn_tl", "crnn", "srres", "edsr"):
    A, calls = sequence(C.module_builder(name, DEV), C.EVAL_SEQ)
    res["eval"][name] = dict(calls=calls, plans=n_plans(A))
for name in ("tsrn", "srres", "edsr"):
    A, calls = sequence(C.step_builder(name, DEV), C.STEP_SEQ)
    res["step"][name] = dict(calls=calls, plans=n_plans(A), static_shape=list(A._static["shape"]))
for stu_iter in (1, 2):
    A, calls = sequence(C.cascade_builder(DEV, stu_iter), C.CASCADE_SEQ)
    res["cascade"][str(stu_iter)] = dict(calls=calls, plans=n_plans(A), static_shape=list(A._static["key"][1]))

# ---- a plan recorded before the shared scratch was regrown keeps the tensors it was recorded against
def pointers(plan):
    from tpgsr_amd import _lib
    return [a for name, fn, args, sid in plan.ops if fn is not None for t, a in zip(fn.argtypes, args) if t is _lib.vp and isinstance(a, int)]

scr = {}
for name, mk in (("tsrn", C.step_builder("tsrn_stn", DEV)), ("crnn", None)):
    if mk is not None:
        ts = mk()
        eng = ts.model._engine()
        ts.step(*C.O.synthetic_batch(4, 1))
        grow = lambda: ts.step(*C.O.synthetic_batch(6, 2))
    else:
        net = C.build_crnn(DEV).train()
        eng = net._engine()
        gray = lambda N: C.MODULES["crnn"][1](N, 3, DEV)[0]
        eng.forward(gray(4), True); eng.backward(4, gray(4), torch.rand(4, 26, 37), need_dgray=True)
        grow = lambda: (eng.forward(gray(6), True), eng.backward(6, gray(6), torch.rand(6, 26, 37), need_dgray=True))
    (entry,) = list(eng._plans.values())
    before = dict(eng._scratch)
    grow()
    regrown = {n: t for n, t in before.items() if eng._scratch[n] is not t}
    used, unkept = 0, []
    for pname, plan in entry.items():
        if not isinstance(plan, K.Plan):
            continue
        ptrs = pointers(plan)
        kept = {t.untyped_storage().data_ptr() for t in plan.keep if isinstance(t, torch.Tensor)}
        for n, t in regrown.items():
            lo, hi = t.data_ptr(), t.data_ptr() + 4 * t.numel()
            if any(lo <= p < hi for p in ptrs):
                used += 1
                if t.untyped_storage().data_ptr() not in kept:
                    unkept.append([pname, n])
    scr[name] = dict(scratch=sorted(before), regrown=sorted(regrown), used=used, unkept=unkept)
res["scratch"] = scr

# ---- a train step keeps the static set of every shape it served; _static is the set of the current shape
def flat(st):
    return [t for v in st.values() for t in (v if isinstance(v, list) else [v]) if isinstance(t, torch.Tensor)]

stat = {}
for name, mk in (("tsrn", C.step_builder("tsrn", DEV)), ("edsr", C.step_builder("edsr", DEV)), ("cascade", C.cascade_builder(DEV, 2))):
    ts = mk()
    ts.step(*C.O.synthetic_batch(4, 1))
    refs = {k: [weakref.ref(t) for t in flat({k: v})] for k, v in ts._static.items()}
    dloss = weakref.ref(ts._static["dloss"])
    ts.step(*C.O.synthetic_batch(6, 2))
    gc.collect()
    dead = sorted(k for k, rs in refs.items() if any(r() is None for r in rs))
    shape6 = list(ts._static["shape"] if "shape" in ts._static else ts._static["key"][1])
    ts.step(*C.O.synthetic_batch(4, 3))
    stat[name] = dict(tensors=sum(len(rs) for rs in refs.values()), released=dead, shape_after_6=shape6,
                      same_set_again=dloss() is not None and ts._static["dloss"] is dloss())
res["statics"] = stat

# ---- refusals
def err(f):
    try:
        f()
    except Exception as e:
        return [type(e).__name__, str(e)]
    return None

ref = {}
for name in ("srres", "edsr"):
    net = C.MODULES[name][0](DEV).train()
    eng = net._engine()
    x4, x6 = (C.MODULES[name][1](N, 5, DEV)[0] for N in (4, 6))
    sr4 = eng.forward(x4, True, slot=0)
    sr6 = eng.forward(x6, True, slot=0)
    ref[name] = dict(stale=err(lambda: eng.backward(tuple(x4.shape), sr4, torch.rand_like(sr4), slot=0)),
                     owner=err(lambda: eng.backward(tuple(x6.shape), sr6, torch.rand_like(sr6), slot=0)),
                     twice=err(lambda: eng.backward(tuple(x6.shape), sr6, torch.rand_like(sr6), slot=0)), saved=len(eng._saved))
res["refusals"] = ref
print("RESULT " + json.dumps(res))
'''


@pytest.fixture(scope="module")
def rec():
    env = dict(os.environ, TPGSR_PLAN_DRYRUN="1")
    for k in [k for k in env if k.startswith("TPGSR_") and k != "TPGSR_PLAN_DRYRUN"]:
        del env[k]
    env["TPGSR_CONV_PREC"] = "x3"                       # (what tests/conftest.py sets for the suite)
    r = subprocess.run([sys.executable, "-c", SCRIPT % dict(root=ROOT, tests=os.path.join(ROOT, "tests"))], capture_output=True, text=True,
                       env=env, timeout=550)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


def _check_calls(calls, seq):
    assert [tuple(c["op"]) for c in calls] == [tuple(op) for op in seq]
    for c in calls:
        print(c)
        assert c["first_difference"] is None and c["lines"] == c["twin_lines"], c
        assert c["plans"] >= 1 or c["lines"] > 20, c          # (the trace is not empty: recorded engines replay plans, the others launch operator by operator)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("name", ["tsrn", "tsrn_tl", "crnn", "srres", "edsr"])
def test_eval_trace_of_each_batch_size_equals_a_fresh_module(rec, name):
    from call_sequence_common import EVAL_SEQ
    got = rec["eval"][name]
    _check_calls(got["calls"], EVAL_SEQ)
    # N = 4, 6, 1 in eval mode: three keys (the plan engines; module(x) of the operator-level backbones runs operator by operator and records none)
    assert got["plans"] == [3 if name in ("tsrn", "tsrn_tl", "crnn") else 0]


@pytest.mark.parametrize("name", ["tsrn", "srres", "edsr"])
def test_train_step_trace_with_interleaved_eval_equals_a_fresh_step(rec, name):
    from call_sequence_common import STEP_SEQ
    got = rec["step"][name]
    _check_calls(got["calls"], STEP_SEQ)
    # training at N = 4, 6, 1 (+ eval at N = 6 for the plan engine; module(x) of srres / EDSR records nothing)
    assert got["plans"] == [4 if name == "tsrn" else 3]
    assert got["static_shape"] == [4, 4, 16, 64]


@pytest.mark.parametrize("stu_iter", [1, 2])
def test_cascade_trace_with_interleaved_evaluator_equals_a_fresh_cascade(rec, stu_iter):
    from call_sequence_common import CASCADE_SEQ
    got = rec["cascade"][str(stu_iter)]
    _check_calls(got["calls"], CASCADE_SEQ)
    # SR net: training N = 4, 6 per stage slot + eval N = 6, 1; each student: training N = 4, 6 in its stage's slot + eval N = 6, 1; the
    # teacher (eval): N = 4, 6 of the steps and N = 6, 1 as the evaluator's recogniser -> 4, 6, 1
    assert got["plans"] == [2 * stu_iter + 2] + [4] * stu_iter + [3]
    assert got["static_shape"] == [4, 4, 16, 64]


@pytest.mark.parametrize("name", ["tsrn", "crnn"])
def test_plan_recorded_before_a_scratch_regrow_keeps_its_scratch(rec, name):
    got = rec["scratch"][name]
    print(got)
    assert got["regrown"] and got["used"] > 0          # (the batch of 6 did replace buffers the batch-of-4 plans point into)
    assert got["unkept"] == []


@pytest.mark.parametrize("name", ["tsrn", "edsr", "cascade"])
def test_step_keeps_the_static_set_of_every_shape_it_served(rec, name):
    """what `capture()` relies on: the graph holds the addresses of the static set of ITS shape, and an eager step at another shape (the
    ragged last batch) must not release it"""
    got = rec["statics"][name]
    print(got)
    assert got["tensors"] >= 5 and got["released"] == []
    assert got["shape_after_6"] == [6, 4, 16, 64]      # _static is the set of the current shape
    assert got["same_set_again"]


@pytest.mark.parametrize("name", ["srres", "edsr"])
def test_functional_engine_refuses_a_backward_whose_slot_was_overwritten(rec, name):
    got = rec["refusals"][name]
    assert got["stale"] is not None and got["stale"][0] == "RuntimeError" and "overwritten" in got["stale"][1], got
    assert got["owner"] is None                        # the forward that owns the slot still gets its backward pass
    assert got["twice"] is not None and got["twice"][0] == "RuntimeError" and got["saved"] == 0
