"""CPU (TPGSR_PLAN_DRYRUN=1): what the train-step drivers of tpgsr_amd/interfaces/super_resolution.py do on the host around the recorded
plans is, line for line, what commit ca45ce0 did -- the last one with two copies of the step skeleton (TSRNTrainStep / TPGSRTrainStep), the
image criterion as a string plus three numbers, and a CRNN engine that read its schedule switches whenever it recorded or was asked.

One trace per step configuration, first and second `step()`: every launch made outside a recording (entry point + a CRC of its scalar
arguments, selected through the C signature as tests/plan_signature.py selects them -- pointers are left out), every `Plan.run` (the plan's
name) and every `GradientExchanger.begin / launch / finish` (the bucket index), in the order they happen; and `[type, message]` of every
refusal of the two classes.

tests/golden/step_trace.json was generated ON ca45ce0, not on the code under test: `python tests/test_step_trace_cpu.py <checkout of
ca45ce0>` runs the SCRIPT below against that tree's package and writes the file (the script needs nothing newer than that commit).

The same script pins the owner of the CRNN backward cut: an engine answers `early_final_offset()` from what it read when it was built, so
a TPGSR_CRNN_BWD_SPLIT that changes after the plans were recorded cannot make the step's bucket bounds disagree with them (on ca45ce0 the
first assertion of test_crnn_cut_has_one_owner fails: the engine re-read the variable and reported None for a pass recorded as two plans)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLD = os.path.join(ROOT, "tests", "golden", "step_trace.json")

SCRIPT = r'''
import json, os, sys, zlib, torch
sys.path[:0] = [%(root)r, %(tests)r]
from oracle import tpgsr_oracle as O
from tpgsr_amd import _lib, kernels as K
assert K.DRYRUN
from plan_signature import fields
from tpgsr_amd.distributed import GradientExchanger
from tpgsr_amd.interfaces.super_resolution import SRTrainStep, TPGSRTrainStep, TSRNTrainStep
from tpgsr_amd.model import lapsrn, rdn, srresnet, tsrn
from tpgsr_amd.model.crnn import crnn

assert SRTrainStep is TSRNTrainStep
lines = []
_launch, _run = K._launch, K.Plan.run

def launch_spy(name, *args):
    if K._REC is None:
        vals = []
        for t, a in zip(getattr(_lib.load(), name).argtypes, args):
            if t in (_lib.ci, _lib.ll, _lib.cf):
                vals.append(round(float(a), 6))
            elif t is not _lib.vp:
                fields(a._obj, vals)
        lines.append("launch %%s %%08x" %% (name, zlib.crc32(repr(vals).encode())))
    return _launch(name, *args)

def run_spy(plan):
    lines.append("plan %%s" %% plan.name)
    return _run(plan)

def exch_spy(what):
    orig = getattr(GradientExchanger, what)
    def spy(self, *b):
        lines.append(" ".join(["exchange", what] + [str(int(x)) for x in b]))
        return orig(self, *b)
    setattr(GradientExchanger, what, spy)

K._launch, K.Plan.run = launch_spy, run_spy
for what in ("begin", "launch", "finish"):
    exch_spy(what)

def two_steps(ts, *batch, **kw):
    out = []
    for _ in range(2):
        del lines[:]
        loss = ts.step(*batch, **kw)
        assert tuple(loss.shape) == ()
        out.append(list(lines))
    return out

def err(f):
    try:
        f()
    except Exception as e:
        return [type(e).__name__, str(e)]
    return None

def cascade(sr_nets, n_stu=1, **kw):
    stus = [crnn.CRNN(32, 1, 37, 256).train() for _ in range(n_stu)]
    return TPGSRTrainStep(sr_nets, stus, crnn.CRNN(32, 1, 37, 256).eval(), **kw), stus

torch.manual_seed(0)
N = 4
lr, hr, hr4 = torch.rand(N, 4, 16, 64), torch.rand(N, 4, 32, 128), torch.rand(N, 4, 64, 256)
tsrn_tl = lambda **kw: tsrn.TSRN_TL(STN=True, mask=True, **kw).train()
srres_tl = lambda: srresnet.SRResNet_TL(scale_factor=2, width=128, height=32, STN=False, mask=True).train()
trace = {}
trace["a_tsrn"] = two_steps(TSRNTrainStep(tsrn.TSRN(STN=True, mask=True).train()), lr, hr)
trace["b_srres_mse"] = two_steps(SRTrainStep(srresnet.SRResNet(mask=True).train(), image_crit="mse"), lr, hr)
trace["c_rdn_l1_rgb"] = two_steps(SRTrainStep(rdn.RDN().train(), image_crit="l1", channels=3), lr, hr)
trace["d_lapsrn_x4_charbonnier_rgb"] = two_steps(SRTrainStep(lapsrn.LapSRN(scale_factor=4).train(), image_crit="l1_charbonnier", channels=3), lr, hr4)
c3, c3_stus = cascade([tsrn_tl()])
trace["e_c3"] = two_steps(c3, lr, hr)
ts, _ = cascade([tsrn_tl()], 2, stu_iter=2, sr_share=True, ssim_loss=True, world_size=1, force_collectives=True)
trace["f_two_stages_ssim_collective"] = two_steps(ts, lr, hr)
ts, _ = cascade([tsrn_tl()], use_label=True)
trace["g_use_label"] = two_steps(ts, lr, hr, labels=O.collate_labels(["a", "ab", "abc", "abcd"]))
ts, _ = cascade([srres_tl()], image_crit="mse")
trace["h_srresnet_tl_mse"] = two_steps(ts, lr, hr)

ref = {}
ref["unknown_crit_single"] = err(lambda: TSRNTrainStep(tsrn.TSRN(STN=True, mask=True), image_crit="charbonnier"))
ref["unknown_crit_cascade"] = err(lambda: cascade([tsrn_tl()], image_crit="charbonnier"))
ref["channels_0"] = err(lambda: SRTrainStep(rdn.RDN().train(), image_crit="l1", channels=0))
ref["channels_5_of_4"] = err(lambda: SRTrainStep(rdn.RDN().train(), image_crit="l1", channels=5).step(lr, hr))
ref["eval_single"] = err(lambda: TSRNTrainStep(tsrn.TSRN(STN=True, mask=True).eval()).step(lr, hr))
def eval_cascade():
    ts, stus = cascade([tsrn_tl()])
    stus[0].eval()
    ts.step(lr, hr)
ref["eval_cascade"] = err(eval_cascade)
ref["wrong_hr_single"] = err(lambda: TSRNTrainStep(tsrn.TSRN(STN=True, mask=True).train()).step(lr, hr4))
ref["wrong_hr_cascade"] = err(lambda: cascade([tsrn_tl()])[0].step(lr, hr[:, :3]))
ref["use_label_without_labels"] = err(lambda: cascade([tsrn_tl()], use_label=True)[0].step(lr, hr))
ref["no_tpg_loss"] = err(lambda: cascade([tsrn_tl()], use_label=False, use_distill=False))
ref["exchange_functional_single"] = err(lambda: SRTrainStep(rdn.RDN().train(), image_crit="l1", channels=3, force_collectives=True))
ref["exchange_functional_cascade"] = err(lambda: cascade([srres_tl()], image_crit="mse", world_size=2))
ref["scales_disagree"] = err(lambda: cascade([tsrn_tl(), tsrn_tl(scale_factor=4)], stu_iter=2, sr_share=False, tpg_share=True)[0].step(lr, hr))

# ---- the CRNN backward cut: decided when the engine is built.  Last in the script: the variable stays changed.
def bwd_plans(eng):
    (pl,) = [pl for pl in eng._plans.values() if "bwd" in pl and len(pl["bwd"])]
    return sorted(k for k in pl if k.startswith("bwd"))
eng = c3_stus[0]._engine()
cut = dict(recorded=eng.early_final_offset(), plans=bwd_plans(eng))
os.environ["TPGSR_CRNN_BWD_SPLIT"] = "0"
cut["after_change"] = eng.early_final_offset()
late = crnn.CRNN(32, 1, 37, 256).train()._engine()
gray = torch.rand(N, 1, 32, 100)
late.forward(gray, True)
late.backward(N, gray, torch.rand(N, 26, 37))
cut["late"] = dict(offset=late.early_final_offset(), plans=bwd_plans(late))
print("RESULT " + json.dumps(dict(trace=trace, refusals=ref, cut=cut)))
'''


def run_script(root=ROOT):
    """`root`: the tree whose package is traced (the golden file: a checkout of ca45ce0); the script and the signature helper are this tree's"""
    env = dict(os.environ, TPGSR_PLAN_DRYRUN="1")
    for k in [k for k in env if k.startswith("TPGSR_") and k != "TPGSR_PLAN_DRYRUN"]:
        del env[k]                                      # the traced schedule is the default one
    r = subprocess.run([sys.executable, "-c", SCRIPT % dict(root=root, tests=os.path.join(ROOT, "tests"))], capture_output=True, text=True,
                       env=env, timeout=550)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


@pytest.fixture(scope="module")
def rec():
    return run_script()


@pytest.fixture(scope="module")
def want():
    return json.load(open(GOLD))


CONFIGS = ("a_tsrn", "b_srres_mse", "c_rdn_l1_rgb", "d_lapsrn_x4_charbonnier_rgb", "e_c3", "f_two_stages_ssim_collective", "g_use_label",
           "h_srresnet_tl_mse")


@pytest.mark.timeout(600)
@pytest.mark.parametrize("cfg", CONFIGS)
def test_step_trace_equals_parent_line_for_line(rec, want, cfg):
    assert sorted(rec["trace"]) == sorted(want["trace"]) == sorted(CONFIGS)
    for k, (got, ref) in enumerate(zip(rec["trace"][cfg], want["trace"][cfg])):
        diff = [(i, a, b) for i, (a, b) in enumerate(zip(got, ref)) if a != b]
        print(cfg, "step", k, len(got), "lines; first differences:", diff[:5])
        assert len(got) == len(ref) and not diff, (cfg, k, len(got), len(ref), diff[:5])
    assert len(rec["trace"][cfg]) == len(want["trace"][cfg]) == 2


REFUSALS = ("unknown_crit_single", "unknown_crit_cascade", "channels_0", "channels_5_of_4", "eval_single", "eval_cascade", "wrong_hr_single",
            "wrong_hr_cascade", "use_label_without_labels", "no_tpg_loss", "exchange_functional_single", "exchange_functional_cascade",
            "scales_disagree")


@pytest.mark.parametrize("case", REFUSALS)
def test_refusal_type_and_message_equal_parent(rec, want, case):
    assert sorted(want["refusals"]) == sorted(REFUSALS)
    assert want["refusals"][case] is not None and len(want["refusals"][case][1]) > 20      # (the fixture holds a refusal, not a pass)
    assert rec["refusals"][case] == want["refusals"][case]


def test_golden_covers_what_it_is_meant_to(want):
    """read from the fixture, so a regenerated one that lost a case fails here"""
    t = want["trace"]
    names = lambda cfg, k=1: [l.split()[1] for l in t[cfg][k] if l.startswith("launch ")]
    assert len(t["a_tsrn"][1]) <= 12 and [l for l in t["a_tsrn"][1] if l.startswith("plan ")] == ["plan tsrn_fwd_pre", "plan tsrn_fwd", "plan tsrn_bwd"]
    assert "tpgsr_image_loss_fwd" in names("b_srres_mse") and "tpgsr_l1_loss_bwd" in names("c_rdn_l1_rgb")
    assert names("c_rdn_l1_rgb").count("tpgsr_copy_strided") == 2
    assert "tpgsr_charbonnier_loss_fwd" in names("d_lapsrn_x4_charbonnier_rgb") and "tpgsr_charbonnier_loss_bwd" in names("d_lapsrn_x4_charbonnier_rgb")
    assert "plan crnn_bwd_b" in t["e_c3"][1] and not any(l.startswith("exchange") for l in t["e_c3"][1])
    f = [l for l in t["f_two_stages_ssim_collective"][1] if l.startswith("exchange")]
    assert f[0] == "exchange begin" and f[-1] == "exchange finish" and len(f) >= 5, f
    assert "tpgsr_ssim" in names("f_two_stages_ssim_collective") and "tpgsr_ssim_bwd" in names("f_two_stages_ssim_collective")
    assert names("g_use_label").count("tpgsr_ctc_loss") == 2
    assert "tpgsr_image_loss_fwd" in names("h_srresnet_tl_mse") and "plan tsrn_fwd" not in t["h_srresnet_tl_mse"][1]
    r = want["refusals"]
    assert r["eval_single"] == ["RuntimeError", "TSRNTrainStep.step needs model.train()"]
    assert r["unknown_crit_single"][1].startswith("TSRNTrainStep: ") and r["unknown_crit_cascade"][1].startswith("TPGSRTrainStep: ")
    assert r["exchange_functional_single"][0] == r["exchange_functional_cascade"][0] == "NotImplementedError"


def test_crnn_cut_has_one_owner(rec):
    cut = rec["cut"]
    assert cut["recorded"] == 370176 and cut["plans"] == ["bwd", "bwd_b"]
    assert cut["after_change"] == cut["recorded"]          # TPGSR_CRNN_BWD_SPLIT=0 set after the recording: the engine's answer stands
    assert (cut["after_change"] is not None) == ("bwd_b" in cut["plans"])
    assert cut["late"] == dict(offset=None, plans=["bwd"])  # an engine built after the change: one backward plan, no early bucket


if __name__ == "__main__":      # regenerate the fixture from a checkout of the commit named above
    res = run_script(os.path.abspath(sys.argv[1]))
    json.dump(dict(trace=res["trace"], refusals=res["refusals"]), open(GOLD, "w"), indent=0, sort_keys=True)
