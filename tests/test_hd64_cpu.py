"""CPU: hidden_units = 64 (the reference's `--hd_u 64`) through the host layers -- plan recording in dry-run mode (TPGSR_PLAN_DRYRUN=1,
tests/test_plan_dryrun_cpu.py), the reference-pinned fixture against the oracle, the state_dict layout, the C ABI -- and the structural
half of "the default path did not move": the recorded plans of the default hidden_units = 32 network, launch for launch."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

# One line per recorded op of every plan of a network: plan key, plan name, op name, stream id and a CRC of every integer / float the
# launch carries (scalar arguments and the non-pointer fields of argument structs: the geometry the launcher derives its grid from).
# Pointers are left out: they differ from run to run.
SIGNATURE = r'''
import json, sys, torch
sys.path[:0] = [%(root)r, %(tests)r]
from tpgsr_amd import kernels as K
assert K.DRYRUN
from tpgsr_amd.model import tsrn
from plan_signature import signature              # (a TSRN entry lists its plans as pack, pre, fwd, bwd)

def record(hidden, tl, stn, N):
    torch.manual_seed(0)
    cls = tsrn.TSRN_TL if tl else tsrn.TSRN
    net = cls(STN=stn, mask=True, hidden_units=hidden).train()
    x = torch.rand(N, 4, 16, 64, requires_grad=True)
    extra = (torch.zeros(N, 37, 1, 26),) if tl else ()
    y = net(x, *extra)
    y.sum().backward()
    net.eval()
    with torch.no_grad():
        z = net(x, *extra)
    assert tuple(y.shape) == tuple(z.shape) == (N, 4, 32, 128)
    return signature(net._engine()._plans)

print("RESULT " + json.dumps({"tl": record(%(hidden)d, True, True, 4), "plain": record(%(hidden)d, False, False, 2)}))
'''


def _signature(hidden):
    env = dict(os.environ, TPGSR_PLAN_DRYRUN="1")
    for k in [k for k in env if k.startswith("TPGSR_") and k != "TPGSR_PLAN_DRYRUN"]:
        del env[k]                                      # the recorded schedule is the default one
    r = subprocess.run([sys.executable, "-c", SIGNATURE % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), hidden=hidden)], capture_output=True, text=True, env=env, timeout=550)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


@pytest.fixture(scope="module")
def sig64():
    return _signature(64)


@pytest.mark.timeout(600)
def test_hd64_plans_record_without_gpu(sig64):
    """train and eval plans of TSRN_TL(hidden_units=64) (STN, mask) and of TSRN(hidden_units=64) record, every launch well-formed"""
    for tag in ("tl", "plain"):
        ops = [l.split()[2] for l in sig64[tag]]
        assert len(ops) > 100, (tag, len(ops))
        # two GruBlocks per residual block, five blocks, a train and an eval plan: every scan goes through the entry point with `hidden`
        assert ops.count("tpgsr_bigru_fwd_u") == 2 * 5 * 2 and ops.count("tpgsr_bigru_bwd_u") == 2 * 5, tag
        assert "tpgsr_bigru_fwd" not in ops and "tpgsr_bigru_bwd" not in ops and "tpgsr_bigru_bwd2" not in ops


def test_hd64_plans_have_no_fused_32_unit_kernels(sig64):
    """the fused projection + scan kernel and the fused GruBlock weight gradient are 32-unit kernels: not in a 64-unit plan"""
    for tag in ("tl", "plain"):
        ops = {l.split()[2] for l in sig64[tag]}
        assert not ops & {"tpgsr_bigru_proj_fwd", "tpgsr_gru_wgrad"}, ops & {"tpgsr_bigru_proj_fwd", "tpgsr_gru_wgrad"}


@pytest.mark.timeout(600)
def test_default_plans_equal_parent_launch_for_launch():
    """hidden_units = 32: kernel names, stream ids, launch geometry and order are those of commit b494a6b, the last one whose
    tpgsr_conv_args carried the 15 fin_* fields of the retired last-workgroup BatchNorm finalize.  The CRCs cover field names, so
    tests/golden/plan_signature_hd32.json is this file's SIGNATURE script run on the tree without those fields; run on b494a6b with
    fields() skipping exactly those names it gives the same 314 + 186 lines, line for line.  b494a6b's own golden in turn pinned the
    commit before the 64-unit scans."""
    want = json.load(open(os.path.join(GOLD, "plan_signature_hd32.json")))
    got = _signature(32)
    for tag in ("tl", "plain"):
        assert len(got[tag]) == len(want[tag]), (tag, len(got[tag]), len(want[tag]))
        diff = [(i, a, b) for i, (a, b) in enumerate(zip(got[tag], want[tag])) if a != b]
        assert not diff, (tag, diff[:5])


def hd64_fixture():
    """the reference-pinned case of tests/golden/make_golden_hd64.py: fixture, recipe weights and seeded inputs"""
    from oracle import tpgsr_oracle as O
    g = np.load(os.path.join(GOLD, "model_tsrn_tl_hd64.npz"), allow_pickle=False)
    spec = O.tsrn_spec(STN=True, mask=True, text_prior=True, srb_nums=5, hidden_units=64)
    sd = O.recipe_state_dict(spec, int(g["weight_seed"]), tps_hw=(16, 64))
    lr, hr = O.synthetic_batch(2, int(g["data_seed"]))
    prior = F.softmax(torch.randn(2, 37, 1, 26, generator=torch.Generator().manual_seed(int(g["prior_seed"]))) * 2, 1)
    return g, sd, lr, hr, prior


def _close(a, b, tol, what=""):
    a, b = torch.as_tensor(np.asarray(a)), torch.as_tensor(np.asarray(b))
    err = (a.double() - b.double()).abs().max().item()
    assert err <= tol * max(1.0, b.double().abs().max().item()), f"{what}: {err:.3e}"


def test_oracle_matches_hd64_fixture():
    """oracle (hidden_units = 64) vs the reference's numbers in tests/golden/model_tsrn_tl_hd64.npz, with the bounds of
    tests/test_oracle_golden.py::test_whole_tsrn (forward 5e-5, loss 1e-5, gradient norms 2e-3)"""
    from oracle import tpgsr_oracle as O
    g, sd, lr, hr, prior = hd64_fixture()
    p = O.as_params(sd)
    y = O.tsrn_forward(p, lr, prior, training=True, stn=True, text_prior=True, explicit_rnn=True)
    _close(y.detach(), g["sr_train"], 5e-5, "train forward")
    loss = O.image_loss(y, hr).mean() * 100
    _close(loss.item(), g["loss"], 1e-5, "loss")
    loss.backward()
    names = json.loads(str(g["grad_names"]))
    gmax = g["grad_norms"].max()
    for n, ref_norm in zip(names, g["grad_norms"]):
        assert abs(p[n].grad.double().norm().item() - ref_norm) <= 2e-3 * max(ref_norm, 1e-3 * gmax), n
    run = torch.cat([p[k].detach().reshape(-1) for k in json.loads(str(g["running_names"]))])
    _close(run, g["running_cat"], 1e-5, "BatchNorm buffers")
    with torch.no_grad():
        y_eval = O.tsrn_forward(O.as_params(sd, False), lr, prior, training=False, text_prior=True)
    _close(y_eval, g["sr_eval"], 5e-5, "eval forward")


def test_state_dict_layout_hd64():
    from tpgsr_amd.model import tsrn
    want = json.load(open(os.path.join(GOLD, "state_dict_layout_hd64.json")))
    sd = tsrn.TSRN_TL(hidden_units=64, srb_nums=5, STN=True, mask=True).state_dict()
    assert {k: list(v.shape) for k, v in sd.items()} == {k: list(v) for k, v in want["tsrn_tl_hd64"]}
    assert [k for k in sd] == [k for k, _ in want["tsrn_tl_hd64"]]


def test_hd64_abi_symbols():
    from tpgsr_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "tpgsr_hip.h")).read()
    for sym in ("tpgsr_bigru_fwd_u", "tpgsr_bigru_bwd_u"):
        assert hasattr(lib, sym), sym
        assert sym in _lib.EXPORTED_SYMBOLS
        assert re.search(r"\bint\s+%s\s*\(" % sym, header), sym
    # the 32-unit entry points keep their signatures (existing tests call them through ctypes)
    assert re.search(r"int tpgsr_bigru_fwd\(const float\* gi, const float\* w_hh[^;]*int N, int H, int W, int axis, float\* h_out, float\* gates[^;]*void\* stream\);", header)


def test_unsupported_hidden_units_is_refused_by_the_host():
    """any U outside {32, 64} raises NotImplementedError naming the supported set, before anything is launched"""
    env = dict(os.environ, TPGSR_PLAN_DRYRUN="1")
    code = ("import sys, torch; sys.path.insert(0, %r)\n"
            "from tpgsr_amd.model import tsrn\n"
            "net = tsrn.TSRN(STN=False, mask=True, hidden_units=48, srb_nums=1).train()\n"
            "try:\n    net(torch.rand(2, 4, 8, 16))\nexcept NotImplementedError as e:\n    print('REFUSED', e)\n") % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "REFUSED" in r.stdout and "32" in r.stdout and "64" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
