"""What tests/test_edsr_gpu.py, tests/test_rrdb_gpu.py and tests/test_lapsrn_gpu.py share: the network-level tests of a prior-free SR backbone
-- fixture comparison, two-step trajectory, recorded plan against the operator-by-operator run, capture and replay against eager steps, the
recorded step against the serial schedule, the x2-against-x3 gates, the evaluator pass -- written once over an `Arch`: one backbone's
constructor, criterion, fixture stem, seed table, batch sizes, float64 restatement and bounds.  The three files keep their test functions
(node ids, docstrings) and everything that is one backbone's own; a body here makes the assertions all three made and hands back the objects
it built, so that a file adds what only its backbone asserts (EDSR's frozen tensors, LapSRN's untouched second stage) behind the call.

The bounds live in `BOUNDS`, once: forward images 1e-4 (of max(1, |y| max)); every parameter-gradient norm 5e-3 (inside check_param_grads of
tests/test_tl_cascade_gpu.py); trajectory: loss 3e-4, clip norm 3e-3, second loss 2e-2; recorded against operator by operator: SR bitwise,
gradients 1e-6; x2 against x3: |dPSNR| < 1e-3 dB, loss 2e-5, clip norm 2e-3; the evaluator: SR 1e-4, |dPSNR| < 1e-5 dB, dSSIM < 1e-7.

A depth-less backbone (LapSRN) passes nb=None: its seed table and batch sizes are keyed by (None, scale) / None and its fixture keys carry no
`nb{nb}_` prefix.  Seeds and float64 restatements come from the generators' modules; the reference is not imported here."""
import dataclasses
import os
import sys
from typing import Callable, Optional

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_edsr as GE  # noqa: E402
import make_golden_lapsrn as GL  # noqa: E402
import make_golden_rrdb as GR  # noqa: E402
from make_golden_next import generic_recipe  # noqa: E402
from oracle import tpgsr_oracle as O  # noqa: E402
from test_tl_cascade_gpu import check_param_grads  # noqa: E402  (the per-parameter rule of tests/test_next_models_gpu.py)

DEV = "cuda"
SCALES = [2, 4]

BOUNDS = dict(fwd=1e-4,                                      # SR images, of max(1, |y| max): fixture, sr_step0, 12x40, the evaluator's
              loss=3e-4, gnorm=3e-3, loss2=2e-2,             # the two-step trajectory, relative
              rec_grad=1e-6,                                 # recorded against operator by operator: the gradient arena (SR: bitwise)
              x2_dpsnr=1e-3, x2_loss=2e-5, x2_gnorm=2e-3,    # the two-term policy (those of tests/test_policy_x2_gpu.py)
              eval_dpsnr=1e-5, eval_dssim=1e-7)              # the evaluator's metrics against the float64 restatement


@dataclasses.dataclass(frozen=True)
class Arch:
    stem: str                           # fixtures: {stem}_x{s}.npz, train_{stem}_x{s}.npz, {stem}_layouts.json
    build: Callable                     # (scale, nb) -> the module, on the host
    crit: str                           # SRTrainStep's image_crit
    forward64: Callable                 # (p, x, scale, nb) -> the generator's float64 restatement
    ssim64: Callable                    # the generator's float64 SSIM (each over the window taps its fixtures were made with)
    seeds: dict                         # (nb, scale) -> (data, weight, upstream-gradient, 12x40 data) seeds
    n: dict                             # nb -> batch size
    n_store: dict                       # scale -> samples of a 16x64 batch whose SR image is stored
    n_small: int
    small_hw: tuple
    eval_n: int
    eval_nb: Optional[int]
    eval_seeds: dict
    depths: tuple                       # (None,) for a depth-less backbone
    nb_small: Optional[int]             # the depth of the plan / capture / schedule tests
    min_plan_ops: int                   # a recorded forward / backward plan holds more ops than this
    trained: Callable = lambda scale: (lambda name: True)      # scale -> (parameter name -> the optimiser moves it)
    set_form: Optional[Callable] = None                        # (net, form): the `form` axis of the tests, where a backbone has one
    channels: int = 3
    bounds: dict = dataclasses.field(default_factory=lambda: BOUNDS)


def _edsr(scale, nb):
    from tpgsr_amd.model import edsr
    return edsr.EDSR(scale_factor=scale, n_resblocks=nb)


def _rrdb(scale, nb):
    from tpgsr_amd.model import esrgan
    return esrgan.RRDBNet(scale_factor=scale, nb=nb)


def _lapsrn(scale, nb):
    from tpgsr_amd.model import lapsrn
    return lapsrn.LapSRN(scale_factor=scale, width=128, height=32, STN=False)


EDSR = Arch(stem="edsr", build=_edsr, crit="l1", forward64=GE.edsr_forward, ssim64=GE.ssim64, seeds=GE.SEEDS, n=GE.N, n_store=GE.N_STORE,
            n_small=GE.N_SMALL, small_hw=GE.SMALL_HW, eval_n=GE.EVAL_N, eval_nb=GE.EVAL_NB, eval_seeds=GE.EVAL_SEEDS, depths=(2, 32), nb_small=2,
            min_plan_ops=10, trained=lambda scale: (lambda name: name not in GE.FROZEN), set_form=lambda net, form: net.set_form(form))
RRDB = Arch(stem="rrdb", build=_rrdb, crit="l1", forward64=GR.rrdb_forward, ssim64=GR.ssim64, seeds=GR.SEEDS, n=GR.N, n_store=GR.N_STORE,
            n_small=GR.N_SMALL, small_hw=GR.SMALL_HW, eval_n=GR.EVAL_N, eval_nb=GR.EVAL_NB, eval_seeds=GR.EVAL_SEEDS, depths=(2, 23), nb_small=2,
            min_plan_ops=20)
LAPSRN = Arch(stem="lapsrn", build=_lapsrn, crit="l1_charbonnier", forward64=lambda p, x, scale, nb: GL.lapsrn_forward(p, x, scale),
              ssim64=GL.ssim64, seeds={(None, s): v for s, v in GL.SEEDS.items()}, n={None: GL.N}, n_store=GL.N_STORE, n_small=GL.N_SMALL,
              small_hw=GL.SMALL_HW, eval_n=GL.EVAL_N, eval_nb=None, eval_seeds=GL.EVAL_SEEDS, depths=(None,), nb_small=None, min_plan_ops=20,
              trained=GL.trained_names)


def _pre(nb):
    return "" if nb is None else f"nb{nb}_"


def _tag(scale, nb, form=None):
    return " ".join(([] if nb is None else [f"nb {nb}"]) + [f"x{scale}"] + ([] if form is None else [form]))


def _rel_to(ref):
    return max(1.0, float(ref.abs().max()))


def load(arch, scale, nb, wseed=None, form=None, dev=None):
    net = arch.build(scale, nb)
    if arch.set_form is not None:
        arch.set_form(net, form)
    net.load_state_dict(generic_recipe(net.state_dict(), arch.seeds[(nb, scale)][1] if wseed is None else wseed), strict=True)
    return net.to(DEV if dev is None else dev)


def make_step(arch, net, precision="x3"):
    from tpgsr_amd.interfaces.super_resolution import SRTrainStep
    return SRTrainStep(net, image_crit=arch.crit, channels=arch.channels, precision=precision)


def _batch(arch, scale, nb):
    return [a.to(DEV) for a in O.synthetic_batch(arch.n[nb], arch.seeds[(nb, scale)][0], scale=scale)]


# ---- 1. against the fixtures (x3) ------------------------------------------------------------------------------------------------------
def check_vs_fixture(arch, scale, nb, golden_dir, form=None):
    """module(x) under autograd: the SR image, the gradient of every parameter the factor trains for the seeded upstream gradient, the
    12x40 eval forward -> the network after its backward pass"""
    from tpgsr_amd import kernels as K
    C, B, tag = arch.channels, arch.bounds, _tag(scale, nb, form)
    g = np.load(os.path.join(golden_dir, f"{arch.stem}_x{scale}.npz"))
    pre = _pre(nb)
    dseed, wseed, gseed, sseed = arch.seeds[(nb, scale)]
    assert [int(s) for s in g[pre + "seeds"]] == [dseed, wseed, gseed, sseed]
    n = arch.n[nb]
    x = O.synthetic_batch(n, dseed, scale=scale)[0][:, :C].contiguous().to(DEV)
    with K.policy("x3"):
        net = load(arch, scale, nb, form=form).train()
        y = net(x)
        yref = torch.tensor(g[pre + "y"])
        e = (y.detach().cpu()[:arch.n_store[scale]] - yref).abs().max().item()
        gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(gseed))
        (y * gy.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        print(f"{tag}: train fwd max err {e:.2e} (|y| max {float(yref.abs().max()):.2f})")
        assert tuple(y.shape) == (n, C, 16 * scale, 64 * scale) and e < B["fwd"] * _rel_to(yref)
        names = [str(k) for k in g[pre + "grad_names"]]
        assert names == [k for k, _ in net.named_parameters()]
        live = np.array([arch.trained(scale)(k) for k in names])
        check_param_grads(tag, net, g[pre + "grad_names"][live], g[pre + "grad_norms"][live], g[pre + "grad_heads"][live])
        net2 = load(arch, scale, nb, form=form).eval()
        with torch.no_grad():
            xs = O.synthetic_batch(arch.n_small, sseed, lr_hw=arch.small_hw, scale=scale)[0][:, :C].contiguous().to(DEV)
            ys = net2(xs)                                   # fully convolutional: 12x40 is no multiple of the 16-row / 64-column tiles
    want = g[pre + "y_small"]
    e = (ys.cpu() - torch.tensor(want)).abs().max().item()
    print(f"   eval 12x40 fwd max err {e:.2e}")
    assert tuple(ys.shape) == want.shape and e < B["fwd"] * max(1.0, float(np.abs(want).max()))
    return net


def check_trajectory(arch, scale, nb, golden_dir, form=None):
    """two steps of the reference loop body through SRTrainStep; the optimiser moves exactly the tensors the factor trains -> (net, step)"""
    from tpgsr_amd.engine_functional import PlainSREngine
    C, B, tag = arch.channels, arch.bounds, _tag(scale, nb, form)
    t = np.load(os.path.join(golden_dir, f"train_{arch.stem}_x{scale}.npz"))
    pre = _pre(nb)
    n = arch.n[nb]
    lr, hr = _batch(arch, scale, nb)
    net = load(arch, scale, nb, form=form).train()
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    ts = make_step(arch, net)
    losses, gns = [], []
    for step in range(2):
        loss = ts.step(lr, hr)
        torch.cuda.synchronize()
        losses.append(loss.item())
        gns.append(ts.opt.grad_norm(net).item())
        if step == 0:
            ref = torch.tensor(t[pre + "sr_step0"])
            e = (ts.last_sr.cpu()[:arch.n_store[scale]] - ref).abs().max().item()
            print(f"   {_tag(scale, nb)}: sr_step0 max err {e:.2e}")
            assert tuple(ts.last_sr.shape) == (n, C, 16 * scale, 64 * scale) and e < B["fwd"] * _rel_to(ref)
    L, G = t[pre + "loss"], t[pre + "gnorm"]
    print(f"{tag} losses {losses} vs {L}; clip norms {gns} vs {G}")
    assert abs(losses[0] - L[0]) < B["loss"] * L[0]
    assert abs(gns[0] - G[0]) < B["gnorm"] * G[0]
    assert abs(losses[1] - L[1]) < B["loss2"] * L[1]
    eng = net._engine()
    assert isinstance(eng, PlainSREngine) and eng.record and eng.scale == scale and len(eng._plans) == 1
    after = net.state_dict()
    for k in before:      # a tensor the factor does not train is bit-identical after two steps, every other one has moved
        assert torch.equal(before[k], after[k]) == (not arch.trained(scale)(k)), k
    return net, ts


# ---- 2. recorded against operator by operator, capture + replay, the serial schedule, the two-term policy ---------------------------
def passes(arch, scale, record, form=None, n_pass=3):
    from tpgsr_amd import kernels as K
    C = arch.channels
    net = load(arch, scale, arch.nb_small, form=form).train()
    eng = net._engine()
    eng.record = record
    n = arch.n[arch.nb_small]
    g = torch.Generator().manual_seed(93)
    outs = []
    with K.policy("x3"):
        for i in range(n_pass):
            lr = torch.rand(n, C, 16, 64, generator=g).to(DEV)
            dsr = torch.randn(n, C, 16 * scale, 64 * scale, generator=g).to(DEV)
            sr = eng.forward(lr, True, slot=i % 2)
            eng.arena.attach_grads()
            eng.arena.grad.zero_()
            assert eng.backward(tuple(lr.shape), sr, dsr, slot=i % 2) is None
            torch.cuda.synchronize()
            outs.append(dict(sr=sr.clone(), grad=eng.arena.grad.clone()))
    return outs, eng


def check_recorded_equals_eager(arch, scale, form=None):
    rec, eng = passes(arch, scale, True, form)
    ref, _ = passes(arch, scale, False, form)
    m = arch.min_plan_ops
    assert len(eng._plans) == 2 and all(len(pl["fwd"]) > m and len(pl["bwd"]) > m for pl in eng._plans.values())
    for i, (a, b) in enumerate(zip(rec, ref)):
        assert torch.equal(a["sr"], b["sr"]), (i, float((a["sr"] - b["sr"]).abs().max()))
        d = (a["grad"] - b["grad"]).abs().max().item()
        assert d <= arch.bounds["rec_grad"] * b["grad"].abs().max().item(), (i, d)


def check_capture_replay(arch, scale, form=None):
    """two replays are bitwise the eager twin's second and third step"""
    nb = arch.nb_small
    lr, hr = _batch(arch, scale, nb)
    net_a, net_b = load(arch, scale, nb, form=form).train(), load(arch, scale, nb, form=form).train()
    ea, eb = make_step(arch, net_a, None), make_step(arch, net_b, None)
    eb.capture(lr, hr, warmup=1)
    la = [ea.step(lr, hr).item() for _ in range(3)]
    lb = [eb.replay().item() for _ in range(2)]
    torch.cuda.synchronize()
    print(la, lb)
    assert lb[0] == la[1] and lb[1] == la[2]
    assert torch.equal(ea.pool.flat, eb.pool.flat)
    assert torch.equal(ea.last_sr, eb.last_sr)


@pytest.fixture()
def schedule():
    from tpgsr_amd import kernels as K
    yield K
    K.set_schedule()          # always back to the default schedule
    torch.cuda.synchronize()


def check_serial_schedule(arch, scale, K, form=None):
    """the default schedule gives the bits of the SAME step replayed in recording order on one stream (fresh networks record their own
    plans in serial mode); K: the `schedule` fixture"""
    nb = arch.nb_small
    lr, hr = _batch(arch, scale, nb)

    def run():
        net = load(arch, scale, nb, form=form).train()
        ts = make_step(arch, net, None)
        losses = [ts.step(lr, hr).item() for _ in range(3)]
        torch.cuda.synchronize()
        return losses, ts.pool.flat.clone(), ts.last_sr.clone()

    la, pa, sa = run()
    K.set_schedule(serial=True)
    lb, pb, sb = run()
    K.set_schedule()
    print(*([] if form is None else [form]), "default", la, "serial", lb)
    assert la == lb
    assert torch.equal(pa, pb) and torch.equal(sa, sb)


def check_two_term_gates(arch, scale, nb, form=None):
    """the step's default policy x2 against x3 on the same batch and weights"""
    B = arch.bounds
    lr, hr = _batch(arch, scale, nb)
    res = {}
    for prec in ("x3", "x2"):
        net = load(arch, scale, nb, form=form).train()
        ts = make_step(arch, net, precision=prec)
        loss = ts.step(lr, hr).item()
        torch.cuda.synchronize()
        res[prec] = (loss, ts.opt.grad_norm(net).item(), ts.last_sr.cpu())
    hr3 = hr.cpu()[:, :arch.channels]
    dpsnr = abs(float(O.calculate_psnr(res["x2"][2], hr3)) - float(O.calculate_psnr(res["x3"][2], hr3)))
    (l3, g3, _), (l2, g2, _) = res["x3"], res["x2"]
    print(f"{_tag(scale, nb, form)}: x2 loss {l2:.6f} vs x3 {l3:.6f}; |dPSNR| {dpsnr:.3e} dB; clip norm {g2:.5f} vs {g3:.5f}")
    assert dpsnr < B["x2_dpsnr"]
    assert abs(l2 - l3) < B["x2_loss"] * l3
    assert abs(g2 - g3) < B["x2_gnorm"] * g3


# ---- 3. the prior-free pass of the evaluator --------------------------------------------------------------------------------------------
def check_evaluator_pass(arch, scale, golden_dir):
    """-> (evaluator, network, the LR batch on the host)"""
    from tpgsr_amd.interfaces.super_resolution import TextSREvaluator
    from tpgsr_amd.model.crnn import crnn
    C, B, nb = arch.channels, arch.bounds, arch.eval_nb
    g = np.load(os.path.join(golden_dir, f"{arch.stem}_x{scale}.npz"))
    lr, hr = O.synthetic_batch(arch.eval_n, int(g["eval_seed"]), scale=scale)
    net = load(arch, scale, nb, arch.eval_seeds[scale]).eval()
    sd = generic_recipe(net.state_dict(), arch.eval_seeds[scale])
    rec = crnn.CRNN(32, 1, 37, 256)
    rec.load_state_dict(O.recipe_state_dict(O.crnn_spec(), arch.eval_seeds["rec"]))
    ev = TextSREvaluator([net], None, recognizer=rec.to(DEV).eval(), channels=C)
    labels = ["abc", "y3", "", "hello", "y3y3", "zz9"]
    out = ev.eval_batch(lr.to(DEV), hr.to(DEV), labels)
    torch.cuda.synchronize()
    with torch.no_grad():
        want = arch.forward64(GL.to64({k: v.cpu() for k, v in sd.items()}), lr[:, :C].double(), scale, nb)
        hr64 = hr[:, :C].double()
        psnr64, ssim_64 = float(O.calculate_psnr(want, hr64)), float(arch.ssim64(want, hr64))
    assert len(out["images_sr"]) == 1 and out["priors"] == []
    sr = out["images_sr"][0]
    sr64 = sr.cpu().double()
    e = (sr64 - want).abs().max().item()
    dp, ds = abs(float(out["psnr"]) - psnr64), abs(float(out["ssim"]) - ssim_64)
    print(f"x{scale}: SR max err {e:.2e}; psnr {float(out['psnr']):.6f} vs {psnr64:.6f} (|d| {dp:.2e} dB); ssim {float(out['ssim']):.8f} vs "
          f"{ssim_64:.8f} (|d| {ds:.2e})")
    # where a metric's deviation comes from: the SR image's own error carried through the float64 metric, against the metric kernel's arithmetic
    print(f"   the image alone (float64 metrics on the device's SR image): |dPSNR| {abs(float(O.calculate_psnr(sr64, hr64)) - psnr64):.2e} dB, "
          f"dSSIM {abs(float(arch.ssim64(sr64, hr64)) - ssim_64):.2e}; mean signed image error {float((sr64 - want).mean()):.2e}")
    assert tuple(sr.shape) == (arch.eval_n, C, 16 * scale, 64 * scale) and e < B["fwd"] * _rel_to(want)
    assert dp < B["eval_dpsnr"]
    assert ds < B["eval_dssim"]
    strings = {k: [str(s) for s in g["eval_" + k]] for k in ("sr", "lr", "hr")}
    assert out["pred_sr"] == strings["sr"] and out["pred_lr"] == strings["lr"] and out["pred_hr"] == strings["hr"]
    assert out["n_correct_sr"] == sum(a == b for a, b in zip(strings["sr"], labels))
    # the HR grid follows the engine's factor: the other factor's HR batch is refused
    other = O.synthetic_batch(arch.eval_n, int(g["eval_seed"]), scale=6 - scale)[1]
    with pytest.raises(ValueError):
        ev.eval_batch(lr.to(DEV), other.to(DEV))
    return ev, net, lr
