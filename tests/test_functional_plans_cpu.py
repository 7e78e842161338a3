"""CPU (TPGSR_PLAN_DRYRUN=1): the recorded plans of the functional engines (tpgsr_amd/engine_functional.py: the `--tpg OPT` recogniser, the
`_TL` backbones, the prior-free baselines) and of the two hand-recorded engines (TSRN_TL, CRNN) are, launch for launch, those of commit
e1602ab -- the last one with three copies of the trace routine in engine_functional.py and with the scheduling flags of a backward plan
(Plan.overlap / deferred / use_leaf) stamped on as ad-hoc attributes at five sites.

tests/golden/plan_signature_functional.json was generated ON e1602ab, not on the code under test: the SCRIPT below, run from a checkout of
that commit (it needs nothing newer than it from the package; tests/plan_signature.py is the signature of tests/test_hd64_cpu.py).  The
networks are the smallest that reach every difference between the three adapters: a student recogniser with d gray, a teacher under
"x2" (the role reaches terms_for), each `_TL` family with two cascade slots and a prior-free eval pass, the three prior-free baselines."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLD = os.path.join(ROOT, "tests", "golden", "plan_signature_functional.json")
sys.path.insert(0, ROOT)

SCRIPT = r'''
import json, sys, torch
sys.path[:0] = [%(root)r, %(tests)r]
from tpgsr_amd import kernels as K
assert K.DRYRUN and K.POLICY == "x3"
import bench
from plan_signature import signature
from tpgsr_amd.model import rdn, srcnn, srresnet, tsrn, vdsr
from tpgsr_amd.model.crnn import crnn, model as opt

N = 2
sig, facts = {}, {}

def seeded(make):
    torch.manual_seed(0)
    return make()

# ---- the `--tpg OPT` recogniser: a student (forward + backward with d gray) and a teacher under "x2"
gray = torch.rand(N, 1, 32, 100)
net = seeded(lambda: opt.Model(bench.OPT_ARGS)).train()
eng = net._engine()
logits = eng.forward(gray, True)
dg = eng.backward(N, gray, torch.randn(N, 26, 37), need_dgray=True)
(pl,) = eng._plans.values()
facts["opt_dgray_is_a_copy"] = dg is not pl["dgray"] and dg.data_ptr() != pl["dgray"].data_ptr() and tuple(dg.shape) == (N, 1, 32, 100)
sig["opt_student"] = signature(eng._plans)
net = seeded(lambda: opt.Model(bench.OPT_ARGS)).eval()
eng = net._engine()
eng.role = "teacher"
with K.policy("x2"):
    eng.forward(gray, False)
sig["opt_teacher_x2"] = signature(eng._plans)

# ---- one `_TL` backbone per family: two cascade slots (forward 0, 1; backward 1, 0), then an eval pass without a prior
TL = {"srresnet_tl": lambda: srresnet.SRResNet_TL(scale_factor=2, width=128, height=32, STN=False, mask=True),
      "srcnn_tl": lambda: srcnn.SRCNN_TL(scale_factor=2, width=128, height=32, STN=False),
      "vdsr_tl": lambda: vdsr.VDSR_TL(scale_factor=2, width=128, height=32, STN=False),
      "rdn_tl": lambda: rdn.RDN_TL(scale_factor=2)}
lr, prior = torch.rand(N, 4, 16, 64), torch.rand(N, 37, 1, 26)
same = []
for name, make in TL.items():
    net = seeded(make).train()
    eng = net._engine()
    srs = [eng.forward(lr, True, prior, slot=s) for s in (0, 1)]
    for s in (1, 0):
        dp = eng.backward(tuple(lr.shape), srs[s], torch.randn_like(srs[s]), slot=s)
        same.append(dp is eng._plans[(tuple(lr.shape), True, s, K.POLICY)]["dprior"])
    net.eval()
    eng.forward(lr, False, None)
    sig[name] = signature(eng._plans)
facts["tl_backward_returns_the_plan_buffer"] = all(same) and len(same) == 8

# ---- the prior-free baselines
PLAIN = {"srres": (lambda: srresnet.SRResNet(scale_factor=2, width=128, height=32, STN=False, mask=True), 4),
         "rdn": (lambda: rdn.RDN(scale_factor=2), 3),
         "vdsr": (lambda: vdsr.VDSR(scale_factor=2, width=128, height=32, STN=False), 3)}
no_prior, returns = [], []
for name, (make, ch) in PLAIN.items():
    net = seeded(make).train()
    eng = net._engine()
    x = torch.rand(N, ch, 16, 64)
    sr = eng.forward(x, True)
    returns.append(eng.backward(tuple(x.shape), sr, torch.randn_like(sr)))
    no_prior += ["prior" not in pl and "dprior" not in pl for pl in eng._plans.values()]
    sig[name] = signature(eng._plans)
facts["plain_plans_have_no_prior"] = all(no_prior) and len(no_prior) == 3
facts["plain_backward_returns_none"] = all(r is None for r in returns)

# ---- the hand-recorded engines: one train step each (their backward plans get their flags from the same constructor)
net = seeded(lambda: tsrn.TSRN_TL(STN=True, mask=True)).train()
net(torch.rand(N, 4, 16, 64, requires_grad=True), torch.zeros(N, 37, 1, 26)).sum().backward()
sig["tsrn_tl"] = signature(net._engine()._plans)
net = seeded(lambda: crnn.CRNN(32, 1, 37, 256)).train()
net(torch.rand(N, 1, 32, 100, requires_grad=True)).sum().backward()
sig["crnn"] = signature(net._engine()._plans)
facts["crnn_backward_is_two_plans"] = any(l.rsplit(" ", 4)[1] == "bwd_b" for l in sig["crnn"])

print("RESULT " + json.dumps(dict(sig=sig, facts=facts)))
'''


def run_script(root=ROOT):
    """`root`: the tree whose package is recorded (the golden file: a checkout of e1602ab); the script and the signature are this tree's"""
    env = dict(os.environ, TPGSR_PLAN_DRYRUN="1")
    for k in [k for k in env if k.startswith("TPGSR_") and k != "TPGSR_PLAN_DRYRUN"]:
        del env[k]                                      # the recorded schedule is the default one
    r = subprocess.run([sys.executable, "-c", SCRIPT % dict(root=root, tests=os.path.join(ROOT, "tests"))], capture_output=True, text=True,
                       env=env, timeout=550)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


@pytest.fixture(scope="module")
def rec():
    return run_script()


@pytest.mark.timeout(600)
def test_plans_equal_parent_launch_for_launch(rec):
    want = json.load(open(GOLD))
    assert sorted(rec["sig"]) == sorted(want)
    for tag in want:
        got = rec["sig"][tag]
        diff = [(i, a, b) for i, (a, b) in enumerate(zip(got, want[tag])) if a != b]
        print(tag, len(got), "lines;", "first differences:", diff[:5])
        assert len(got) == len(want[tag]) and not diff, (tag, len(got), len(want[tag]), diff[:5])


def test_golden_covers_every_row_of_the_adapters(rec):
    """what the fixture pins (read from the fixture, so a regenerated one that lost a case fails here)"""
    want = json.load(open(GOLD))
    cols = lambda l: l.rsplit(" ", 4)                  # key (may hold blanks), plan, op, stream id, CRC
    plans = lambda tag: {tuple(cols(l)[:2]) for l in want[tag]}
    assert {p for _, p in plans("opt_student")} == {"fwd", "bwd"} and {p for _, p in plans("opt_teacher_x2")} == {"fwd"}
    assert all(cols(l)[0] == "2/False/0/teacher/x2" for l in want["opt_teacher_x2"])
    for tag in ("srresnet_tl", "srcnn_tl", "vdsr_tl", "rdn_tl"):
        keys = {k for k, _ in plans(tag)}
        assert keys == {"(2, 4, 16, 64)/True/0/x3", "(2, 4, 16, 64)/True/1/x3", "(2, 4, 16, 64)/False/0/x3"}, keys
    for tag in ("srres", "rdn", "vdsr"):
        assert {p for _, p in plans(tag)} == {"fwd", "bwd"}
    assert {"bwd", "bwd_b", "fwd"} <= {p for _, p in plans("crnn")} and "bwd" in {p for _, p in plans("tsrn_tl")}
    for tag in want:                                   # weight gradients on their own stream, joined: the default flags were read
        if tag != "opt_teacher_x2":
            assert any(cols(l)[2] == "fork" for l in want[tag]) and any(cols(l)[3] == "1" for l in want[tag]), tag


def test_what_backward_returns(rec):
    f = rec["facts"]
    assert f["plain_plans_have_no_prior"] and f["plain_backward_returns_none"]
    assert f["tl_backward_returns_the_plan_buffer"]          # FunctionalSREngine.backward: the very tensor pl["dprior"], no copy
    assert f["opt_dgray_is_a_copy"]                          # the recogniser's backward: a fresh tensor, not pl["dgray"]
    assert f["crnn_backward_is_two_plans"]


# ---- Plan owns its scheduling flags ----------------------------------------------------------------------------------------------------
def _record_sections(plan):
    """a side and a leaf section around one launch each, recorded into `plan` (raw addresses: nothing runs, as in tests/test_abi_cpu.py);
    the stream ids of the recorded launches and the stream dependencies in between"""
    from tpgsr_amd import kernels as K
    with K.recording(plan):
        with K.side():
            K._launch("tpgsr_zero", 0x1000, 16)
        with K.leaf():
            K._launch("tpgsr_zero", 0x2000, 16)
        K._REC.join()
    return [op[3] for op in plan.ops if op[1] is not None], [op[0] for op in plan.ops if op[1] is None]


def test_fresh_plan_records_serially():
    from tpgsr_amd import kernels as K
    plan = K.Plan("p")
    assert plan.overlap is False and plan.deferred is None and plan.use_leaf is False
    sids, edges = _record_sections(plan)
    assert sids == [0, 0] and edges == []               # nothing on streams 1 / 2, no fork / edge / join
    with K.recording(plan):
        assert not K.deferring()


def test_backward_plan_reads_the_environment_at_call_time(monkeypatch):
    from tpgsr_amd import kernels as K
    monkeypatch.delenv("TPGSR_OVERLAP_WGRAD", raising=False)
    monkeypatch.delenv("TPGSR_DEFER_REDUCE", raising=False)
    p = K.backward_plan("b")
    assert p.name == "b" and p.overlap is True and p.deferred == [] and p.use_leaf is False
    assert _record_sections(p) == ([1, 0], ["fork", "join"])                   # (leaf sections need use_leaf)
    assert _record_sections(K.backward_plan("b", use_leaf=True)) == ([1, 2], ["fork", "edge", "edge", "join"])
    monkeypatch.setenv("TPGSR_OVERLAP_WGRAD", "0")
    p = K.backward_plan("b", use_leaf=True)
    assert p.overlap is False and p.deferred == [] and _record_sections(p) == ([0, 0], [])
    monkeypatch.setenv("TPGSR_DEFER_REDUCE", "0")
    p = K.backward_plan("b")
    assert p.overlap is False and p.deferred is None
    # explicit arguments win over the environment
    p = K.backward_plan("b", overlap=True, defer=True)
    assert p.overlap is True and p.deferred == []
    monkeypatch.setenv("TPGSR_OVERLAP_WGRAD", "1")
    monkeypatch.setenv("TPGSR_DEFER_REDUCE", "1")
    p = K.backward_plan("b", overlap=False, defer=False)
    assert p.overlap is False and p.deferred is None
    a, b = K.backward_plan("a"), K.backward_plan("b")
    assert a.deferred is not b.deferred                 # each plan collects its own reduces
