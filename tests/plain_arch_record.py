"""What tests/test_edsr_cpu.py, tests/test_rrdb_cpu.py and tests/test_lapsrn_cpu.py share: the dry-run child (TPGSR_PLAN_DRYRUN=1) that records
one `SRTrainStep` and one evaluator pass per case of a prior-free backbone without a GPU, and the checks whose assertions are the same for
all three -- the C ABI of new entry points, the criterion's kernels, the evaluator pass, the committed fixtures.  A file hands `record` its
backbone's import line, its cases (loops over forms and scales that call `train_case` / `eval_case` of the child) and an optional extra
block; the kernel counts per plan are each backbone's own and stay in its file."""
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLD = os.path.join(ROOT, "tests", "golden")

RECORD = r'''
import json, sys, torch
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
from tpgsr_amd import kernels as K
assert K.DRYRUN
from tpgsr_amd import functional as Fh
from tpgsr_amd.engine_functional import PlainSREngine
from tpgsr_amd.interfaces.super_resolution import SRTrainStep, TextSREvaluator
from tpgsr_amd.model.crnn import crnn
from plan_signature import signature
%(imports)s

direct = []
_launch = K._launch
def spy(name, *a):
    if K._REC is None:
        direct.append(name)
    return _launch(name, *a)
K._launch = spy

def err(f):
    try:
        f()
    except Exception as e:
        return [type(e).__name__, str(e)]
    return None

def train_case(make_net, s, crit):
    """one dry-run step of SRTrainStep over make_net(): the recorded plan, the launches next to it, the refusal of a wrong HR grid"""
    del direct[:]
    net = make_net().train()
    ts = SRTrainStep(net, precision="x3", image_crit=crit, channels=3)
    loss = ts.step(torch.rand(4, 4, 16, 64), torch.rand(4, 4, 16 * s, 64 * s))
    eng = net._engine()
    assert isinstance(eng, PlainSREngine) and eng.record and tuple(loss.shape) == ()
    (key, pl), = eng._plans.items()
    lines = signature(eng._plans)                 # runs every plan: the native executor checks entry point and argument count of every op
    a, b = ts.pool.ranges[id(net)]
    return dict(key=[str(k) for k in key], fwd=[o[0] for o in pl["fwd"].ops], bwd=[o[0] for o in pl["bwd"].ops], direct=list(direct),
                sr=list(ts.last_sr.shape), scale=eng.scale, nsig=len(lines),
                pooled=bool(eng.arena.external is not None and b - a == eng.arena.numel),
                sunk=all(p.grad is not None for p in net.parameters()), has_prior=("prior" in pl or "dprior" in pl),
                wrong_hr=err(lambda: ts.step(torch.rand(4, 4, 16, 64), torch.rand(4, 4, 8 * s, 32 * s))))

recognizer = crnn.CRNN(32, 1, 37, 256).eval()
def eval_case(make_net, s):
    """the prior-free evaluator pass over make_net(): its one recorded forward plan and the launches next to it"""
    del direct[:]
    net = make_net().eval()
    ev = TextSREvaluator([net], None, recognizer=recognizer, channels=3)
    srs, priors = ev.super_resolve(torch.rand(6, 4, 16, 64))
    (pl,) = net._engine()._plans.values()
    return dict(direct=list(direct), sr=list(srs[0].shape), priors=len(priors), plan=[o[0] for o in pl["fwd"].ops])

NB = 2
out = {}
torch.manual_seed(0)
%(cases)s
%(extra)s
print("RESULT " + json.dumps(out))
'''


def record(imports, cases, extra=""):
    """run the child under TPGSR_PLAN_DRYRUN=1 with every other TPGSR_* variable stripped -> its RESULT dictionary"""
    env = dict(os.environ, TPGSR_PLAN_DRYRUN="1")
    for k in [k for k in env if k.startswith("TPGSR_") and k != "TPGSR_PLAN_DRYRUN"]:
        del env[k]
    script = RECORD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), imports=imports, cases=cases, extra=extra)
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, env=env, timeout=550)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


def check_entry_points(symbols, source=None, n_structs=13):
    """every symbol exported, declared in the header, registered with the plan executor and bound with scalar and pointer parameters only
    (no new argument block: n_structs); source: the .hip file the build has to list"""
    from tpgsr_amd import _lib
    from tpgsr_amd.build import SOURCES
    header = open(os.path.join(ROOT, "include", "tpgsr_hip.h")).read()
    plan = open(os.path.join(ROOT, "tpgsr_amd", "csrc", "plan.cpp")).read()
    assert source is None or source in SOURCES
    for sym in symbols:
        assert sym in _lib.EXPORTED_SYMBOLS
        assert re.search(r"\bint\s+%s\s*\(" % sym, header)
        assert "TPGSR_REG(%s)" % sym in plan
        fn = getattr(_lib.load(), sym)
        assert len(fn.argtypes) <= 24 + 1
    assert len(_lib.ABI_STRUCTS) == n_structs


# image_crit -> (kernels a step launches next to its plan, kernels of the other criteria it must not)
CRITERION_KERNELS = {
    "l1": (("tpgsr_l1_loss_fwd", "tpgsr_l1_loss_bwd"), ("tpgsr_charbonnier_loss_fwd", "tpgsr_image_loss_fwd")),
    "l1_charbonnier": (("tpgsr_charbonnier_loss_fwd", "tpgsr_charbonnier_loss_bwd", "tpgsr_image_loss_finalize"),
                       ("tpgsr_image_loss_fwd", "tpgsr_l1_loss_fwd", "tpgsr_image_loss_bwd")),
}


def check_criterion_kernels(rec, keys, crit):
    present, absent = CRITERION_KERNELS[crit]
    for k in keys:
        d = rec[k]["direct"]
        assert all(name in d for name in present) and not any(name in d for name in absent), (k, d)
        assert d.count("tpgsr_copy_strided") == 2          # channels=3: the RGB prefixes of LR and HR


def check_evaluator_case(r, s):
    """one recorded forward plan behind the channel-prefix copy: no text-prior launch next to it"""
    assert r["sr"] == [6, 3, 16 * s, 64 * s] and r["priors"] == 0
    assert r["direct"] == ["tpgsr_copy_strided", "tpgsr_copy", "tpgsr_copy"]


def check_fixtures(arch, scale):
    """the committed fixtures of an Arch of tests/plain_arch_common.py: sizes, shapes, finite values, the module's parameter names, and a
    gradient norm of zero exactly for the tensors the factor does not train"""
    for path in (f"{arch.stem}_x{scale}.npz", f"train_{arch.stem}_x{scale}.npz", f"{arch.stem}_layouts.json"):
        assert os.path.getsize(os.path.join(GOLD, path)) < 700 * 1000, path
    g = np.load(os.path.join(GOLD, f"{arch.stem}_x{scale}.npz"), allow_pickle=False)
    t = np.load(os.path.join(GOLD, f"train_{arch.stem}_x{scale}.npz"), allow_pickle=False)
    for nb in arch.depths:
        pre = "" if nb is None else f"nb{nb}_"
        assert g[pre + "y"].shape == t[pre + "sr_step0"].shape == (min(arch.n_store[scale], arch.n[nb]), 3, 16 * scale, 64 * scale)
        assert g[pre + "y_small"].shape == (arch.n_small, 3, 12 * scale, 40 * scale)
        assert t[pre + "loss"].shape == (2,) and t[pre + "gnorm"].shape == (2,) and (t[pre + "loss"] > 0).all() and (t[pre + "gnorm"] > 0).all()
        for k in ("y", "y_small", "grad_norms", "grad_heads"):
            assert np.isfinite(g[pre + k]).all() and g[pre + k].size, k
        names = [n for n, _ in arch.build(scale, nb).named_parameters()]
        assert [str(n) for n in g[pre + "grad_names"]] == names
        for n, v in zip(names, g[pre + "grad_norms"]):
            assert (v > 0) if arch.trained(scale)(n) else (v == 0), n      # the reference computes no gradient for an untrained tensor
    assert len(g["eval_sr"]) == len(g["eval_lr"]) == len(g["eval_hr"]) == 6
