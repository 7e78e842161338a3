"""CPU (TPGSR_PLAN_DRYRUN=1): one forward and one backward of every PARAMETERISED operator of tpgsr_amd/functional.py, recorded launch for
launch, equals commit d97b637 -- the last one on which each of these operators carried its own copy of the parameter-gradient protocol
(slabs, side section, sink lookup, accumulate or allocate) -- and under a recording with sinks no operator hands autograd a gradient.

tests/golden/plan_signature_ops.json was generated ON d97b637, not on the code under test: the SCRIPT below, run from a checkout of that
commit (`run_script(root=<checkout>)["sig"]`, without the "bigru-*/b" entries; it needs nothing newer than it from the package, and
tests/plan_signature.py gives the line format).  Each operator is recorded under the policies "x3" and "f32" (the fused res_block takes
another branch without bf16 twins) in two ways:
  a  forward and backward into fresh `K.Plan`s, no sinks: the eager launch sequence;
  b  the backward into a `K.backward_plan` (weight gradients on stream 1, slab reduces deferred into one program) with a sink for every
     parameter: what a FunctionalEngine trace records.  The deferred reduces are lines too: `<key> bwd deferred acc=<accumulate> <CRC>`.
All of (a), and (b) of every operator but bigru, are compared with the fixture.  The two BiGRU operators ignored the sinks on d97b637 (their
gradients went through autograd once, at trace time, and every replay left them out), so their (b) is asserted structurally instead."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLD = os.path.join(ROOT, "tests", "golden", "plan_signature_ops.json")

SCRIPT = r'''
import json, sys, types, zlib, torch
sys.path[:0] = [%(root)r, %(tests)r]
from tpgsr_amd import functional as Fh, kernels as K
assert K.DRYRUN and K.POLICY == "x3"
from plan_signature import signature

def bn(C):
    return types.SimpleNamespace(weight=torch.ones(C), bias=torch.zeros(C), running_mean=torch.zeros(C), running_var=torch.ones(C),
                                 momentum=0.1, eps=1e-5, num_batches_tracked=torch.tensor(0))

def gru(Cin, U):
    names = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
    shapes = ((3 * U, Cin), (3 * U, U), (3 * U,), (3 * U,))
    return types.SimpleNamespace(**{n + suf: torch.zeros(*s) for suf in ("", "_reverse") for n, s in zip(names, shapes)})

def dense_w(nf, gc):
    return [torch.zeros(nf if k == 4 else gc, nf + k * gc, 3, 3) for k in range(5)], [torch.zeros(nf if k == 4 else gc) for k in range(5)]

# name -> (input shape, the parameters, op(x, *parameters)); holders (BatchNorm, GRU) list their parameter tensors
def cases():
    C = {}
    w, b = torch.zeros(16, 8, 3, 3), torch.zeros(16)
    C["conv2d-bias"] = ((1, 3, 5, 8), [w, b], lambda x, w, b: Fh.conv2d(x, w, b, 1))
    C["conv2d-nobias"] = ((1, 3, 5, 8), [w], lambda x, w: Fh.conv2d(x, w, None, 1))
    C["conv2d-wscale"] = ((1, 3, 5, 8), [w, b], lambda x, w, b: Fh.conv2d(x, w, b, 1, wscale=0.5))
    C["linear"] = ((3, 5, 8), [torch.zeros(12, 8), torch.zeros(12)], lambda x, w, b: Fh.linear(x, w, b))
    C["conv_transpose2d"] = ((1, 3, 5, 8), [torch.zeros(8, 4, 3, 3)], lambda x, w: Fh.conv_transpose2d(x, w, 2, 1))
    for form, c in (("direct", 3), ("subpixel", 64), ("dilated", 8)):
        C["tconv_k4s2-" + form] = ((1, 3, 5, c), [torch.zeros(c, c, 4, 4)], lambda x, w, form=form: Fh.conv_transpose2d_k4s2(x, w, form=form))
    h = bn(8)
    C["batch_norm"] = ((1, 3, 5, 8), [h.weight, h.bias], lambda x, *_, h=h: Fh.batch_norm(x, h, True, "relu"))
    C["prelu"] = ((1, 3, 5, 8), [torch.full((1,), 0.25)], lambda x, a: Fh.prelu(x, a))
    ws, bs = dense_w(8, 4)
    for form in Fh.DENSE_FORMS:
        C["dense_block-" + form] = ((1, 3, 5, 8), ws + bs, lambda x, *p, form=form: Fh.dense_block(x, p[:5], p[5:], form=form))
    w1, w2 = torch.zeros(8, 8, 3, 3), torch.zeros(8, 8, 3, 3)
    for form in Fh.RES_FORMS:
        C["res_block-" + form] = ((1, 3, 5, 8), [w1, w2], lambda x, w1, w2, form=form: Fh.res_block(x, w1, w2, form=form))
    for form in Fh.NARROW_FORMS:
        C["conv2d_narrow-" + form] = ((1, 3, 5, 8), [torch.zeros(3, 8, 3, 3)], lambda x, w, form=form: Fh.conv2d_narrow(x, w, form=form))
    for U in (32, 64):
        for axis in (0, 1):
            h = gru(64, U)
            C["bigru-U%%d-axis%%d" %% (U, axis)] = ((1, 2, 5, 64), list(vars(h).values()), lambda x, *_, h=h, axis=axis: Fh.bigru(x, h, axis))
    return C

class sinks_installed:      # (by hand: the script also records d97b637, which has no functional.grad_sinks)
    def __init__(self, table):
        self.table = table
    def __enter__(self):
        self.prev, Fh.GRAD_SINK = Fh.GRAD_SINK, self.table
    def __exit__(self, *exc):
        Fh.GRAD_SINK = self.prev
        return False

def record(name, mode):
    shape, params, op = cases()[name]                     # fresh tensors for every recording
    x = torch.zeros(*shape).requires_grad_(True)
    hooked = []
    for p in params:
        p.requires_grad_(True)
        p.register_hook(lambda g, hooked=hooked: hooked.append(g is not None))      # what the operator handed autograd for p
    fwd = K.Plan("fwd")
    with K.recording(fwd):
        y = op(x, *params)
    dy = torch.zeros_like(y)
    deferred = []
    if mode == "a":
        bwd = K.Plan("bwd")
        with K.recording(bwd):
            torch.autograd.backward(y, dy)
    else:
        bwd = K.backward_plan("bwd")
        with sinks_installed({p.data_ptr(): torch.zeros_like(p) for p in params}), K.recording(bwd):
            torch.autograd.backward(y, dy)
            deferred = list(bwd.deferred)
            K.flush_wgrad_reduces()
            K._REC.join()
    key = (name, K.POLICY, mode)
    lines = signature({key: dict(fwd=fwd, bwd=bwd)})
    for part, dbpart, Z, Kd, Cin, Cout, KH, KW, layout, dw, db, acc, gscale, cin_ld, leaf in deferred:
        vals = [Z, Kd, Cin, Cout, KH, KW, layout, round(float(gscale), 6), cin_ld, int(dbpart is not None), int(db is not None), int(leaf)]
        lines.append("%%s bwd deferred acc=%%d %%08x" %% ("/".join(key), acc, zlib.crc32(repr(vals).encode())))
    facts = dict(params=len(params), handed=sum(hooked), grads=sum(p.grad is not None for p in params))
    return "/".join(key), lines, facts

sig, facts = {}, {}
for pol in ("x3", "f32"):
    with K.policy(pol):
        for name in cases():
            for mode in "ab":
                key, sig[key], facts[key] = record(name, mode)
print("RESULT " + json.dumps(dict(sig=sig, facts=facts)))
'''


def run_script(root=ROOT):
    """`root`: the tree whose package is recorded (the golden file: a checkout of d97b637); the script and the signature are this tree's"""
    env = dict(os.environ, TPGSR_PLAN_DRYRUN="1")
    for k in [k for k in env if k.startswith("TPGSR_") and k != "TPGSR_PLAN_DRYRUN"]:
        del env[k]                                      # the recorded schedule is the default one
    r = subprocess.run([sys.executable, "-c", SCRIPT % dict(root=root, tests=os.path.join(ROOT, "tests"))], capture_output=True, text=True,
                       env=env, timeout=280)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


@pytest.fixture(scope="module")
def rec():
    return run_script()


def cols(line):
    return line.rsplit(" ", 4)                          # key, plan, op, stream id (deferred lines: acc=<flag>), CRC


def is_gru_b(key):
    return key.startswith("bigru-") and key.endswith("/b")


OPS = ["conv2d-bias", "conv2d-nobias", "conv2d-wscale", "linear", "conv_transpose2d", "tconv_k4s2-direct", "tconv_k4s2-subpixel",
       "tconv_k4s2-dilated", "batch_norm", "prelu", "dense_block-inplace", "dense_block-composed", "res_block-fused", "res_block-composed",
       "conv2d_narrow-narrow", "conv2d_narrow-matrix", "bigru-U32-axis0", "bigru-U32-axis1", "bigru-U64-axis0", "bigru-U64-axis1"]


def test_every_operator_is_recorded(rec):
    keys = {f"{op}/{pol}/{mode}" for op in OPS for pol in ("x3", "f32") for mode in "ab"}
    assert set(rec["sig"]) == keys
    assert set(json.load(open(GOLD))) == {k for k in keys if not is_gru_b(k)}


def test_launches_equal_parent_launch_for_launch(rec):
    want = json.load(open(GOLD))
    for key in want:
        got = rec["sig"][key]
        diff = [(i, a, b) for i, (a, b) in enumerate(zip(got, want[key])) if a != b]
        assert len(got) == len(want[key]) and not diff, (key, len(got), len(want[key]), diff[:5])


def test_golden_pins_the_protocol():
    """read from the fixture, so a regenerated one that lost a case fails here: without sinks nothing leaves stream 0 and no reduce is
    deferred; with them every operator's parameter gradient runs on stream 1 or accumulates (BatchNorm's finalize and PReLU's reduce stay on
    stream 0 by design) and every deferred reduce accumulates"""
    want = json.load(open(GOLD))
    for key, lines in want.items():
        c = [cols(l) for l in lines]
        if key.endswith("/a"):
            assert all(x[3] == "0" and x[2] not in ("fork", "join", "deferred") for x in c), key
            continue
        assert all(x[3] == "acc=1" for x in c if x[2] == "deferred"), key
        if not key.startswith(("batch_norm", "prelu")):
            assert any(x[2] == "fork" for x in c) and any(x[3] == "1" for x in c) and c[-1][2] in ("join", "deferred"), key
    assert any(cols(l)[2] == "deferred" for l in want["conv2d-bias/x3/b"])
    assert not any(cols(l)[2] == "deferred" for l in want["tconv_k4s2-subpixel/x3/b"])          # reduced at once: the fold reads it
    assert want["res_block-fused/x3/b"] != [l.replace("/f32/", "/x3/") for l in want["res_block-fused/f32/b"]]


def test_sunk_gradients_never_reach_autograd(rec):
    """under a recording with sinks every operator -- the BiGRU included -- hands autograd None for each parameter, so no AccumulateGrad
    runs that a replay would miss; without sinks every parameter gets its gradient from autograd"""
    for key, f in rec["facts"].items():
        assert f["params"] > 0
        if key.endswith("/b"):
            assert f["handed"] == 0 and f["grads"] == 0, (key, f)
        else:
            assert f["handed"] == f["params"] == f["grads"], (key, f)


def test_bigru_under_sinks(rec):
    """(b) of the BiGRU operators: the launches of (a), with the four weight gradients on stream 1 and their four slab reduces deferred into
    one program there, each with accumulate = 1"""
    for key in filter(is_gru_b, rec["sig"]):
        a = [cols(l) for l in rec["sig"][key[:-1] + "a"]]
        b = [cols(l) for l in rec["sig"][key]]
        launches = lambda c, drop: [(x[1], x[2], x[4]) for x in c if x[2] not in ("fork", "join", "edge", "deferred", drop)]
        assert launches(a, "tpgsr_wgrad_reduce") == launches(b, "tpgsr_wgrad_reduce_program"), key
        assert sum(x[2] == "tpgsr_wgrad_reduce" for x in a) == 4 and not any(x[2] == "tpgsr_wgrad_reduce" for x in b), key
        wg = [x for x in b if x[2] == "tpgsr_conv_wgrad"]
        assert len(wg) == 4 and all(x[3] == "1" for x in wg), key
        assert [x[3] for x in b if x[2] == "tpgsr_wgrad_reduce_program"] == ["1"], key
        assert [x[3] for x in b if x[2] == "deferred"] == ["acc=1"] * 4, key
        assert all(x[3] == "0" for x in b if x[1] == "bwd" and x[2].startswith("tpgsr_") and x[2] not in
                   ("tpgsr_conv_wgrad", "tpgsr_wgrad_reduce_program")), key
        assert [x[2] for x in b if x[2] in ("fork", "join")].count("join") == 1 and b[-5][2] == "join", key
