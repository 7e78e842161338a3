"""GPU: `--arch edsr` (EDSR x2 / x4, nn.L1Loss) -- functional.res_block in both forms, the module operator by operator and through
`SRTrainStep` + engine_functional.PlainSREngine against fixtures generated from the reference's own module
(tests/golden/make_golden_edsr.py); FusedAdam over the frozen MeanShift tensors; recorded plans against the operator-by-operator run on
fresh inputs, hipGraph capture, the recorded step under the serial schedule (the side-stream reads of res_scale * dy and dz), the two-term
policy, batch independence, the prior-free evaluator pass.

Bounds: those of tests/test_rrdb_gpu.py for the same quantities -- forward images 1e-4 (of max(1, |y| max)), every parameter-gradient
norm 5e-3 (check_param_grads), trajectory: loss 3e-4, clip norm 3e-3, second loss 2e-2; recorded against operator by operator: SR
bitwise, gradients 1e-6; x2 against x3: |dPSNR| < 1e-3 dB, loss 2e-5, clip norm 2e-3.  The evaluator: SR 1e-4, |dPSNR| < 1e-5 dB and
dSSIM < 1e-7 against the float64 restatement, identical strings.  res_block: the fused form against the composed one within 1e-6 (of the
composed result's largest magnitude) under the default policy x3; both against float64 autograd under the `arith` rule of
tests/kernel_table.py (e_gpu <= 4 * e_ref32 + 4 * 2^-24) under policy f32, where the fused form's data gradient has no activation epilogue
and tpgsr_act_bwd runs behind it.  The block's inputs come from the first seed of BLOCK_SEEDS whose float64 pre-activations all keep
|conv1(x)| >= KINK_MARGIN: an element within float32 rounding of the ReLU's kink has derivative 0 in one arithmetic and 1 in another, and
no bound on arithmetic covers that (the pattern of POOL_SEEDS in tests/test_functional_ops_gpu.py).  One image alone against its row of a
batch: 1e-5 of max(1, |y| max) -- the convolution launches of a batch of one may split their contraction (fewer tiles than compute
units), which re-associates float32 sums of seven layers at 2^-24 each; leakage between images would be of order 1."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_golden_edsr import (CHANNELS, EVAL_N, EVAL_NB, EVAL_SEEDS, FROZEN, N, N_SMALL, N_STORE, SEEDS, SMALL_HW, edsr_forward, ssim64,  # noqa: E402
                              to64)      # (seeds and the float64 restatement only; the reference is not imported here)
from make_golden_next import generic_recipe  # noqa: E402
from kernel_table import FLOOR, _gen, err  # noqa: E402
from oracle import tpgsr_oracle as O  # noqa: E402
from test_tl_cascade_gpu import check_param_grads  # noqa: E402  (the per-parameter rule of tests/test_next_models_gpu.py)

DEV = "cuda"
SCALES = [2, 4]
DEPTHS = [2, 32]


FORMS = ["fused", "composed"]      # the residual blocks' form (EDSR.set_form): the network-level tests run both, whichever is the default


def load(scale, nb, wseed=None, form=None):
    from tpgsr_amd.model import edsr
    net = edsr.EDSR(scale_factor=scale, n_resblocks=nb)
    net.set_form(form)
    net.load_state_dict(generic_recipe(net.state_dict(), SEEDS[(nb, scale)][1] if wseed is None else wseed), strict=True)
    return net.to(DEV)


def make_step(net, precision="x3"):
    from tpgsr_amd.interfaces.super_resolution import SRTrainStep
    return SRTrainStep(net, image_crit="l1", channels=CHANNELS, precision=precision)


# ---- 0. functional.res_block ---------------------------------------------------------------------------------------------------------
C = 256
RES_SCALE = 0.1
BLOCK_SEEDS = tuple(range(16))
KINK_MARGIN = 2e-6      # ~10x the float32 accumulation error of a 2304-term sum of products of magnitude 0.02


@functools.lru_cache(maxsize=None)
def _block_inputs(hw):
    for seed in BLOCK_SEEDS:
        g = _gen("res_block", hw, seed)
        x = torch.randn(2, hw[0], hw[1], C, generator=g)
        w1, w2 = [torch.randn(C, C, 3, 3, generator=g) / (9 * C) ** 0.5 for _ in range(2)]
        gy = torch.randn(2, hw[0], hw[1], C, generator=g)
        pre = F.conv2d(x.double().permute(0, 3, 1, 2), w1.double(), padding=1)
        if float(pre.abs().min()) >= KINK_MARGIN:
            print(f"res_block {hw}: seed {seed}, min |conv1(x)| {float(pre.abs().min()):.2e}")
            return x, w1, w2, gy
    raise RuntimeError("no seed keeps the pre-activations off the ReLU's kink")


@functools.lru_cache(maxsize=None)
def _block_ref(hw, dtype):
    """stock PyTorch autograd in `dtype` (NHWC in, NHWC out): y, dx, dw1, dw2"""
    x, w1, w2, gy = _block_inputs(hw)
    x = x.to(dtype).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    w1, w2 = [w.detach().clone().to(dtype).requires_grad_(True) for w in (w1, w2)]
    y = F.conv2d(F.relu(F.conv2d(x, w1, padding=1)), w2, padding=1) * torch.tensor(RES_SCALE, dtype=torch.float32).to(dtype) + x
    (y * gy.to(dtype).permute(0, 3, 1, 2)).sum().backward()
    return [y.detach().permute(0, 2, 3, 1), x.grad.permute(0, 2, 3, 1), w1.grad, w2.grad]


def _block_gpu(hw, form):
    from tpgsr_amd import functional as Fh
    x, w1, w2, gy = _block_inputs(hw)
    x = x.to(DEV).requires_grad_(True)
    w1, w2 = [w.to(DEV).requires_grad_(True) for w in (w1, w2)]
    y = Fh.res_block(x, w1, w2, RES_SCALE, form=form)
    (y * gy.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return [t.detach().cpu() for t in (y, x.grad, w1.grad, w2.grad)]


KEYS = ["y", "dx", "dw1", "dw2"]
HWS = [(5, 7), (16, 64)]
HW_IDS = ["5x7", "16x64"]


@pytest.mark.parametrize("hw", HWS, ids=HW_IDS)
def test_res_block_fused_equals_composed(hw):
    from tpgsr_amd import kernels as K
    with K.policy("x3"):
        a, b = _block_gpu(hw, "fused"), _block_gpu(hw, "composed")
    for k, u, v in zip(KEYS, a, b):
        e = err(u, v)
        print(f"{hw} {k}: fused against composed {e:.2e}")
        assert tuple(u.shape) == tuple(v.shape) and e <= 1e-6, (k, e)


@pytest.mark.parametrize("form", ["fused", "composed"])
@pytest.mark.parametrize("hw", HWS, ids=HW_IDS)
def test_res_block_against_float64(hw, form):
    from tpgsr_amd import kernels as K
    r64, r32 = _block_ref(hw, torch.float64), _block_ref(hw, torch.float32)
    with K.policy("f32"):
        got = _block_gpu(hw, form)
    for k, g, a, b in zip(KEYS, got, r64, r32):
        e_gpu, e32 = err(g, a), err(b, a)
        bound = 4 * e32 + FLOOR
        print(f"{form} {hw} {k}: e_gpu {e_gpu:.2e}  e_ref32 {e32:.2e}  bound {bound:.2e}")
        assert tuple(g.shape) == tuple(a.shape) and e_gpu <= bound, (form, k, e_gpu, bound)


def test_res_block_refusals_and_defaults():
    from tpgsr_amd import functional as Fh
    x = torch.zeros(1, 5, 7, 8, device=DEV)
    w = torch.zeros(8, 8, 3, 3, device=DEV)
    with pytest.raises(ValueError, match="form"):
        Fh.res_block(x, w, w, form="inplace")
    with pytest.raises(ValueError, match="channels"):
        Fh.res_block(x, torch.zeros(12, 12, 3, 3, device=DEV), w)
    with pytest.raises(ValueError, match="3x3"):
        Fh.res_block(x, w, torch.zeros(8, 8, 1, 1, device=DEV))
    with pytest.raises(ValueError, match="multiple of 4"):
        Fh.res_block(torch.zeros(1, 5, 7, 6, device=DEV), torch.zeros(6, 6, 3, 3, device=DEV), torch.zeros(6, 6, 3, 3, device=DEV), form="fused")
    assert Fh.RES_DEFAULT_FORM in Fh.RES_FORMS and Fh.NARROW_DEFAULT_FORM in Fh.NARROW_FORMS


# ---- 1. against the fixtures (x3) ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nb", DEPTHS)
@pytest.mark.parametrize("scale", SCALES)
def test_edsr_vs_reference_fixture(scale, nb, form, golden_dir):
    """module(x) under autograd: the SR image, every parameter gradient for the seeded upstream gradient, the 12x40 eval forward"""
    from tpgsr_amd import kernels as K
    g = np.load(os.path.join(golden_dir, f"edsr_x{scale}.npz"))
    pre = f"nb{nb}_"
    dseed, wseed, gseed, sseed = SEEDS[(nb, scale)]
    assert [int(s) for s in g[pre + "seeds"]] == [dseed, wseed, gseed, sseed]
    n = N[nb]
    x = O.synthetic_batch(n, dseed, scale=scale)[0][:, :CHANNELS].contiguous().to(DEV)
    with K.policy("x3"):
        net = load(scale, nb, form=form).train()
        y = net(x)
        yref = torch.tensor(g[pre + "y"])
        sc = max(1.0, float(yref.abs().max()))
        e = (y.detach().cpu()[:N_STORE[scale]] - yref).abs().max().item()
        gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(gseed))
        (y * gy.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        print(f"nb {nb} x{scale} {form}: train fwd max err {e:.2e} (|y| max {float(yref.abs().max()):.2f})")
        assert tuple(y.shape) == (n, CHANNELS, 16 * scale, 64 * scale) and e < 1e-4 * sc
        names = [str(k) for k in g[pre + "grad_names"]]
        assert names == [k for k, _ in net.named_parameters()]
        P = dict(net.named_parameters())
        for k in FROZEN:                                   # no gradient is ever computed for a frozen tensor
            assert P[k].grad is None or float(P[k].grad.abs().max()) == 0.0, k
        live = [i for i, k in enumerate(names) if k not in FROZEN]
        assert len(live) == len(names) - 4
        check_param_grads(f"nb {nb} x{scale} {form}", net, g[pre + "grad_names"][live], g[pre + "grad_norms"][live], g[pre + "grad_heads"][live])
        net2 = load(scale, nb, form=form).eval()
        with torch.no_grad():
            xs = O.synthetic_batch(N_SMALL, sseed, lr_hw=SMALL_HW, scale=scale)[0][:, :CHANNELS].contiguous().to(DEV)
            ys = net2(xs)                                   # fully convolutional: 12x40 is no multiple of the 16-row / 64-column tiles
    want = g[pre + "y_small"]
    e = (ys.cpu() - torch.tensor(want)).abs().max().item()
    print(f"   eval 12x40 fwd max err {e:.2e}")
    assert tuple(ys.shape) == want.shape and e < 1e-4 * max(1.0, float(np.abs(want).max()))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nb", DEPTHS)
@pytest.mark.parametrize("scale", SCALES)
def test_edsr_train_step_vs_reference_trajectory(scale, nb, form, golden_dir):
    """two steps of the reference loop body (interfaces/super_resolution.py:409-424 with nn.L1Loss, torch.optim.Adam over
    model.parameters()) through SRTrainStep: FusedAdam walks the whole arena and leaves the four MeanShift tensors bit for bit"""
    from tpgsr_amd.engine_functional import PlainSREngine
    t = np.load(os.path.join(golden_dir, f"train_edsr_x{scale}.npz"))
    pre = f"nb{nb}_"
    n = N[nb]
    lr, hr = [a.to(DEV) for a in O.synthetic_batch(n, SEEDS[(nb, scale)][0], scale=scale)]
    net = load(scale, nb, form=form).train()
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    ts = make_step(net)
    losses, gns = [], []
    for step in range(2):
        loss = ts.step(lr, hr)
        torch.cuda.synchronize()
        losses.append(loss.item())
        gns.append(ts.opt.grad_norm(net).item())
        if step == 0:
            ref = torch.tensor(t[pre + "sr_step0"])
            e = (ts.last_sr.cpu()[:N_STORE[scale]] - ref).abs().max().item()
            print(f"   nb {nb} x{scale}: sr_step0 max err {e:.2e}")
            assert tuple(ts.last_sr.shape) == (n, CHANNELS, 16 * scale, 64 * scale) and e < 1e-4 * max(1.0, float(ref.abs().max()))
    L, G = t[pre + "loss"], t[pre + "gnorm"]
    print(f"nb {nb} x{scale} {form} losses {losses} vs {L}; clip norms {gns} vs {G}")
    assert abs(losses[0] - L[0]) < 3e-4 * L[0]
    assert abs(gns[0] - G[0]) < 3e-3 * G[0]
    assert abs(losses[1] - L[1]) < 2e-2 * L[1]
    eng = net._engine()
    assert isinstance(eng, PlainSREngine) and eng.record and eng.scale == scale and len(eng._plans) == 1
    after = net.state_dict()
    for k in before:
        assert torch.equal(before[k], after[k]) == (k in FROZEN), k
    for k in FROZEN:                                      # ... and their slices of the gradient arena were never written
        assert float(dict(net.named_parameters())[k].grad.abs().max()) == 0.0, k


def test_fused_adam_still_refuses_an_undeclared_frozen_parameter():
    net = load(2, 2).train()
    net.conv_mid.weight.requires_grad = False
    with pytest.raises(NotImplementedError, match="conv_mid.weight"):
        make_step(net)


# ---- 2. recorded against operator by operator, capture + replay, the serial schedule, the two-term policy ---------------------------
NB_SMALL = 2


def _passes(scale, form, record, n_pass=3):
    from tpgsr_amd import kernels as K
    net = load(scale, NB_SMALL, form=form).train()
    eng = net._engine()
    eng.record = record
    n = N[NB_SMALL]
    g = torch.Generator().manual_seed(93)
    outs = []
    with K.policy("x3"):
        for i in range(n_pass):
            lr = torch.rand(n, CHANNELS, 16, 64, generator=g).to(DEV)
            dsr = torch.randn(n, CHANNELS, 16 * scale, 64 * scale, generator=g).to(DEV)
            sr = eng.forward(lr, True, slot=i % 2)
            eng.arena.attach_grads()
            eng.arena.grad.zero_()
            assert eng.backward(tuple(lr.shape), sr, dsr, slot=i % 2) is None
            torch.cuda.synchronize()
            outs.append(dict(sr=sr.clone(), grad=eng.arena.grad.clone()))
    return outs, eng


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("scale", SCALES)
def test_recorded_plan_equals_operator_by_operator_run(scale, form):
    rec, eng = _passes(scale, form, True)
    ref, _ = _passes(scale, form, False)
    assert len(eng._plans) == 2 and all(len(pl["fwd"]) > 10 and len(pl["bwd"]) > 10 for pl in eng._plans.values())
    for i, (a, b) in enumerate(zip(rec, ref)):
        assert torch.equal(a["sr"], b["sr"]), (i, float((a["sr"] - b["sr"]).abs().max()))
        d = (a["grad"] - b["grad"]).abs().max().item()
        assert d <= 1e-6 * b["grad"].abs().max().item(), (i, d)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("scale", SCALES)
def test_capture_replay_equals_eager_steps(scale, form):
    """two replays are bitwise the eager twin's second and third step"""
    lr, hr = [a.to(DEV) for a in O.synthetic_batch(N[NB_SMALL], SEEDS[(NB_SMALL, scale)][0], scale=scale)]
    net_a, net_b = load(scale, NB_SMALL, form=form).train(), load(scale, NB_SMALL, form=form).train()
    ea, eb = make_step(net_a, None), make_step(net_b, None)
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


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("scale", SCALES)
def test_recorded_step_equals_serial_schedule(scale, form, schedule):
    """the weight-gradient launches of a residual block read res_scale * dy and dz on the side stream while the caller's stream moves on,
    conv_output's partial sums are reduced into the arena there: the default schedule must give the bits of the SAME step replayed in
    recording order on one stream (depth 2, N 4; fresh networks record their own plans in serial mode)"""
    K = schedule
    lr, hr = [a.to(DEV) for a in O.synthetic_batch(N[NB_SMALL], SEEDS[(NB_SMALL, scale)][0], scale=scale)]

    def run():
        net = load(scale, NB_SMALL, form=form).train()
        ts = make_step(net, None)
        losses = [ts.step(lr, hr).item() for _ in range(3)]
        torch.cuda.synchronize()
        return losses, ts.pool.flat.clone(), ts.last_sr.clone()

    la, pa, sa = run()
    K.set_schedule(serial=True)
    lb, pb, sb = run()
    K.set_schedule()
    print(form, "default", la, "serial", lb)
    assert la == lb
    assert torch.equal(pa, pb) and torch.equal(sa, sb)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("scale,nb", [(4, 2), (2, 32)])
def test_two_term_policy_holds_the_gates(scale, nb, form):
    """the step's default policy x2 against x3 on the same batch and weights, with the bounds tests/test_policy_x2_gpu.py sets:
    |dPSNR| < 1e-3 dB, loss within 2e-5, gradient norm within 2e-3"""
    lr, hr = [a.to(DEV) for a in O.synthetic_batch(N[nb], SEEDS[(nb, scale)][0], scale=scale)]
    res = {}
    for prec in ("x3", "x2"):
        net = load(scale, nb, form=form).train()
        ts = make_step(net, precision=prec)
        loss = ts.step(lr, hr).item()
        torch.cuda.synchronize()
        res[prec] = (loss, ts.opt.grad_norm(net).item(), ts.last_sr.cpu())
    hr3 = hr.cpu()[:, :CHANNELS]
    dpsnr = abs(float(O.calculate_psnr(res["x2"][2], hr3)) - float(O.calculate_psnr(res["x3"][2], hr3)))
    (l3, g3, _), (l2, g2, _) = res["x3"], res["x2"]
    print(f"nb {nb} x{scale} {form}: x2 loss {l2:.6f} vs x3 {l3:.6f}; |dPSNR| {dpsnr:.3e} dB; clip norm {g2:.5f} vs {g3:.5f}")
    assert dpsnr < 1e-3
    assert abs(l2 - l3) < 2e-5 * l3
    assert abs(g2 - g3) < 2e-3 * g3


@pytest.mark.parametrize("scale", SCALES)
def test_one_image_alone_equals_its_row_of_the_batch(scale):
    from tpgsr_amd import kernels as K
    x = O.synthetic_batch(3, SEEDS[(NB_SMALL, scale)][0], scale=scale)[0][:, :CHANNELS].contiguous().to(DEV)
    net = load(scale, NB_SMALL).eval()
    with K.policy("x3"), torch.no_grad():
        yb = net(x)
        for j in range(3):
            yj = net(x[j:j + 1].contiguous())
            e = float((yj[0] - yb[j]).abs().max())
            print(f"x{scale} image {j}: alone against row {j} of the batch {e:.2e} (|y| max {float(yb.abs().max()):.2f})")
            assert e <= 1e-5 * max(1.0, float(yb.abs().max())), (j, e)


# ---- 3. the prior-free pass of the evaluator --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", SCALES)
def test_evaluator_pass(scale, golden_dir):
    from tpgsr_amd.interfaces.super_resolution import TextSREvaluator
    from tpgsr_amd.model.crnn import crnn
    g = np.load(os.path.join(golden_dir, f"edsr_x{scale}.npz"))
    lr, hr = O.synthetic_batch(EVAL_N, int(g["eval_seed"]), scale=scale)
    net = load(scale, EVAL_NB, EVAL_SEEDS[scale]).eval()
    sd = generic_recipe(net.state_dict(), EVAL_SEEDS[scale])
    rec = crnn.CRNN(32, 1, 37, 256)
    rec.load_state_dict(O.recipe_state_dict(O.crnn_spec(), EVAL_SEEDS["rec"]))
    ev = TextSREvaluator([net], None, recognizer=rec.to(DEV).eval(), channels=CHANNELS)
    labels = ["abc", "y3", "", "hello", "y3y3", "zz9"]
    out = ev.eval_batch(lr.to(DEV), hr.to(DEV), labels)
    torch.cuda.synchronize()
    with torch.no_grad():
        want = edsr_forward(to64({k: v.cpu() for k, v in sd.items()}), lr[:, :CHANNELS].double(), scale, EVAL_NB)
        hr64 = hr[:, :CHANNELS].double()
        psnr64, ssim_64 = float(O.calculate_psnr(want, hr64)), float(ssim64(want, hr64))
    assert len(out["images_sr"]) == 1 and out["priors"] == []
    sr = out["images_sr"][0]
    e = (sr.cpu().double() - want).abs().max().item()
    dp, ds = abs(float(out["psnr"]) - psnr64), abs(float(out["ssim"]) - ssim_64)
    print(f"x{scale}: SR max err {e:.2e}; psnr {float(out['psnr']):.6f} vs {psnr64:.6f} (|d| {dp:.2e} dB); ssim {float(out['ssim']):.8f} vs "
          f"{ssim_64:.8f} (|d| {ds:.2e})")
    assert tuple(sr.shape) == (EVAL_N, CHANNELS, 16 * scale, 64 * scale) and e < 1e-4 * max(1.0, float(want.abs().max()))
    assert dp < 1e-5
    assert ds < 1e-7
    strings = {k: [str(s) for s in g["eval_" + k]] for k in ("sr", "lr", "hr")}
    assert out["pred_sr"] == strings["sr"] and out["pred_lr"] == strings["lr"] and out["pred_hr"] == strings["hr"]
    assert out["n_correct_sr"] == sum(a == b for a, b in zip(strings["sr"], labels))
    # the HR grid follows the engine's factor: the other factor's HR batch is refused
    other = O.synthetic_batch(EVAL_N, int(g["eval_seed"]), scale=6 - scale)[1]
    with pytest.raises(ValueError):
        ev.eval_batch(lr.to(DEV), other.to(DEV))
