"""GPU: scale_factor = 4 in TSRN / TSRN_TL -- two up-sampling stages (conv3x3 C -> 4C, pixel-shuffle store, mish) in front of the folded 9x9
tail, LR 16x64 -> SR 64x256 -- against the float64 oracle (tests/x4_common.py restates the step-level functions with a scale) and the
reference-pinned fixtures of tests/golden/make_golden_x4.py.

Shapes: N = 3, LR 5x18 leaves ragged 64-pixel tiles at every resolution (270 / 1080 / 4320 pixels, SR 20x72); 16x64 is the smallest input
the STN head admits.  Every bound is the one the x2 sibling uses for the same quantity (tests/test_tsrn_gpu.py, test_fullsize_gpu.py,
test_crnn_gpu.py, test_eval_gpu.py, test_policy_x2_gpu.py; the `4 e_ref32 + 4 * 2^-24` rule of tests/kernel_table.py for the bicubic kernels);
with the STN on, element-wise comparisons carry the STN siblings' bounds (the TPS system's fp32 conditioning)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import tpgsr_oracle as O  # noqa: E402
import x4_common as X  # noqa: E402

DEV = "cuda"
F64 = torch.float64
UP_AND_TAIL = ("block8.0.conv.weight", "block8.0.conv.bias", "block8.1.conv.weight", "block8.1.conv.bias", "block8.2.weight", "block8.2.bias")


def _threads():
    try:
        n = len(os.sched_getaffinity(0))
    except Exception:
        n = os.cpu_count() or 1
    torch.set_num_threads(max(1, min(n, 16)))


def _psnr(a, b):
    return float(O.calculate_psnr(a.detach().cpu().double(), b.detach().cpu().double()))


# ---- the three network cases, float64 reference computed once -----------------------------------------------------------------------
CASES = {
    "tl_stn": dict(tl=True, stn=True, mask=True, N=2, hw=(16, 64)),          # = the fixture's case (tests/golden/model_tsrn_tl_x4.npz)
    "tl_nostn": dict(tl=True, stn=False, mask=True, N=3, hw=(5, 18)),
    "plain3_nostn": dict(tl=False, stn=False, mask=False, N=3, hw=(5, 18)),
}


def _inputs(name):
    c = CASES[name]
    if name == "tl_stn":
        _, sd, lr, hr, prior = X.model_fixture()
        return sd, lr, hr, prior
    kw = dict(scale_factor=4, width=256, height=64, STN=c["stn"], mask=c["mask"])
    sd = O.recipe_state_dict(O.tsrn_spec(text_prior=c["tl"], srb_nums=5, **kw), 400 + len(name), tps_hw=(16, 64))
    lr, hr = O.synthetic_batch(c["N"], 40 + len(name), mask=c["mask"], lr_hw=c["hw"], scale=4)
    prior = X.prior_from_seed(c["N"], 4 + len(name)) if c["tl"] else None
    return sd, lr, hr, prior


@functools.lru_cache(maxsize=None)
def _reference(name):
    """float64 oracle: eval forward, train forward, loss, every parameter gradient, the prior's gradient, BatchNorm buffers after the pass"""
    _threads()
    c = CASES[name]
    sd, lr, hr, prior = _inputs(name)
    lr64, hr64 = lr.double(), hr.double()
    with torch.no_grad():
        y_eval = O.tsrn_forward(X.params(sd, False), lr64, None if prior is None else prior.double(), training=False, stn=c["stn"],
                                text_prior=c["tl"], scale_factor=4)
    p = X.params(sd)
    pr = None if prior is None else prior.double().requires_grad_(True)
    y = O.tsrn_forward(p, lr64, pr, training=True, stn=c["stn"], text_prior=c["tl"], scale_factor=4)
    loss = O.image_loss(y, hr64).mean() * 100
    loss.backward()
    assert y.dtype == F64
    return dict(y_eval=y_eval, y=y.detach(), loss=loss.item(), grads={k: p[k].grad for k in O.trainable_keys(p)},
                dprior=None if pr is None else pr.grad, running={k: v.detach() for k, v in p.items() if "running_" in k})


def _net(name, sd=None):
    from tpgsr_amd.model import tsrn
    c = CASES[name]
    sd = _inputs(name)[0] if sd is None else sd
    cls = tsrn.TSRN_TL if c["tl"] else tsrn.TSRN
    net = cls(scale_factor=4, width=256, height=64, STN=c["stn"], mask=c["mask"])
    net.load_state_dict(sd, strict=True)
    return net.to(DEV)


@pytest.mark.parametrize("name", list(CASES))
def test_x4_forward_vs_float64_oracle(name, golden_policy):
    """eval forward: tol(5e-5) (test_tsrn_tl_vs_golden); train forward: tol(5e-5) without the STN (test_three_channel_network_vs_oracle's
    last_sr: 5e-5 under x3, eight times that under x2 -- measured under x2: 6.1e-5, over the unscaled 5e-5), 5e-3 with it
    (test_tsrn_tl_vs_golden); loss tol(3e-4) (STN, test_tsrn_tl_vs_golden) / tol(1e-4) (test_three_channel_network_vs_oracle)"""
    from tpgsr_amd.loss.image_loss import ImageLoss
    c, ref = CASES[name], _reference(name)
    sd, lr, hr, prior = _inputs(name)
    args = (lr.to(DEV),) + ((prior.to(DEV),) if c["tl"] else ())
    net = _net(name, sd).eval()
    with torch.no_grad():
        y_eval = net(*args)
    s = net._engine().scale
    assert s == 4 and tuple(y_eval.shape) == (c["N"], 4 if c["mask"] else 3, 4 * c["hw"][0], 4 * c["hw"][1])
    e_eval = (y_eval.cpu().double() - ref["y_eval"]).abs().max().item()
    net.train()
    with torch.no_grad():
        y = net(*args)
    e_train = (y.cpu().double() - ref["y"]).abs().max().item()
    loss = (ImageLoss(gradient=True, loss_weight=[1, 1e-4])(y, hr.to(DEV)).mean() * 100).item()
    print(f"x4 {name} {golden_policy.name}: eval fwd err {e_eval:.2e}, train fwd err {e_train:.2e}, loss {loss:.6f} vs {ref['loss']:.6f}")
    assert e_eval < golden_policy.tol(5e-5)
    assert e_train < (5e-3 if c["stn"] else golden_policy.tol(5e-5))
    assert abs(loss - ref["loss"]) < golden_policy.tol(3e-4 if c["stn"] else 1e-4) * abs(ref["loss"])
    if name == "tl_stn":          # the reference's own numbers: lattice and per-image sums (n elements each within the forward bound)
        g = X.model_fixture()[0]
        n = y[0].numel()
        assert (y_eval.cpu()[:, :, ::4, ::4] - torch.tensor(g["sr_eval_lattice"])).abs().max() < golden_policy.tol(5e-5)
        assert (y.cpu()[:, :, ::4, ::4] - torch.tensor(g["sr_train_lattice"])).abs().max() < 5e-3
        se, st = X.image_sums(y_eval.cpu()), X.image_sums(y.cpu())
        assert np.abs(se[:, 0] - g["sr_eval_sums"][:, 0]).max() < golden_policy.tol(5e-5) * n
        assert np.abs(se[:, 1] - g["sr_eval_sums"][:, 1]).max() < 2 * golden_policy.tol(5e-5) * n
        assert np.abs(st[:, 0] - g["sr_train_sums"][:, 0]).max() < 5e-3 * n and np.abs(st[:, 1] - g["sr_train_sums"][:, 1]).max() < 1e-2 * n
        assert abs(loss - float(g["loss"])) < golden_policy.tol(3e-4) * float(g["loss"])


@pytest.mark.parametrize("name", list(CASES))
def test_x4_gradients_vs_float64_autograd(name):
    """every parameter gradient, the prior's gradient, the BatchNorm running buffers.  Without the STN element-wise: |got - ref|_2 <= 2e-3
    max(|ref|_2, 1e-3 gmax) per tensor (test_tsrn_tl_gradients_vs_oracle_nostn), prior 2e-3.  With the STN per-tensor norms, the prior's
    too, to 2e-2 (test_tsrn_tl_vs_golden: one flipped pooling window of the STN head re-routes gradient elements; the element-wise form
    of the STN case is test_x4_same_grid_elementwise_vs_float64).  Buffers 2e-4 (test_tsrn_forward_backward_vs_golden)."""
    from tpgsr_amd.loss.image_loss import ImageLoss
    c, ref = CASES[name], _reference(name)
    sd, lr, hr, prior = _inputs(name)
    net = _net(name, sd).train()
    pd = prior.to(DEV).requires_grad_(True) if c["tl"] else None
    sr = net(lr.to(DEV), pd) if c["tl"] else net(lr.to(DEV))
    loss = ImageLoss(gradient=True, loss_weight=[1, 1e-4])(sr, hr.to(DEV)).mean() * 100
    loss.backward()
    torch.cuda.synchronize()
    gmax = max(v.norm().item() for v in ref["grads"].values())
    bad, named, worst = [], {}, 0.0
    for n, q in net.named_parameters():
        r, got = ref["grads"][n], q.grad.cpu().double()
        if c["stn"]:
            rel = abs(got.norm().item() - r.norm().item()) / max(r.norm().item(), 1e-3 * gmax)
            lim = 2e-2
        else:
            rel = (got - r).norm().item() / max(r.norm().item(), 1e-3 * gmax)
            lim = 2e-3
        worst = max(worst, rel)
        if n in UP_AND_TAIL:
            named[n] = rel
        if rel > lim:
            bad.append((n, rel))
    print(f"x4 {name} gradients: worst {worst:.2e} (bound {lim:.0e}); up-sampling convs and tail:",
          {k: f"{v:.2e}" for k, v in named.items()})
    assert len(named) == len(UP_AND_TAIL)
    assert not bad, (bad[:10], "up-sampling convs / tail:", named)
    if c["tl"] and not c["stn"]:
        rel = (pd.grad.cpu().double() - ref["dprior"]).norm().item() / ref["dprior"].norm().item()
        print(f"x4 {name} dprior rel err {rel:.2e}")
        assert rel < 2e-3
    elif c["tl"]:          # (element-wise with the STN on: test_x4_same_grid_elementwise_vs_float64)
        rel = abs(pd.grad.cpu().double().norm().item() - ref["dprior"].norm().item()) / ref["dprior"].norm().item()
        print(f"x4 {name} dprior norm rel err {rel:.2e}")
        assert rel < 2e-2
    bufs = dict(net.named_buffers())
    e_run = max((bufs[k].detach().cpu().double() - v).abs().max().item() for k, v in ref["running"].items())
    print(f"x4 {name} BatchNorm running buffers err {e_run:.2e}")
    assert e_run < 2e-4


def test_x4_same_grid_elementwise_vs_float64():
    """The STN case (TSRN_TL, N = 2, 16x64) element-wise, the way tests/test_tsrn_gpu.py::test_tsrn_same_grid_elementwise_vs_oracle does it at
    x2 and with its bounds: the float64 oracle is fed the BUILD'S OWN sampling grid as a leaf.
      stage B (everything downstream of the grid): rectified image 2e-6, SR image 5e-5, loss 1e-4, every non-STN parameter gradient and the
              prior's gradient element-wise to 2e-3, the grid's gradient to 2e-3;
      stage A (the STN head): the oracle's head + TPS back-propagate stage B's grid gradient: control-point gradient 5e-3, the head's
              parameter gradients per tensor 2e-2 * NOISE (five max-pools)."""
    from tpgsr_amd.loss.image_loss import ImageLoss
    NOISE = 1.5            # tests/test_tsrn_gpu.py
    _threads()
    sd, lr, hr, prior = _inputs("tl_stn")
    net = _net("tl_stn", sd).train()
    pd = prior.to(DEV).requires_grad_(True)
    sr = net(lr.to(DEV), pd)
    loss = ImageLoss(gradient=True, loss_weight=[1, 1e-4])(sr, hr.to(DEV)).mean() * 100
    loss.backward()
    torch.cuda.synchronize()
    ws = next(pl["ws"].t for key, pl in net._engine()._plans.items() if key[3] and "stn_dgrid" in pl["ws"].t)
    N, H, W = 2, 16, 64
    grid_b = ws["stn_grid"].cpu().reshape(N, H, W, 2).double().clone()
    lr64, hr64 = lr.double(), hr.double()
    # ---- stage B
    p = X.params(sd)
    gl = grid_b.clone().requires_grad_(True)
    pr = prior.double().requires_grad_(True)
    xr = F.grid_sample(lr64, gl, mode="bilinear", padding_mode="zeros", align_corners=False)
    y = O.tsrn_forward(p, xr, pr, training=True, stn=False, text_prior=True, scale_factor=4)
    loss_ref = O.image_loss(y, hr64).mean() * 100
    loss_ref.backward()
    e_xr = (ws["xr"].cpu().reshape(N, H, W, 4).permute(0, 3, 1, 2).double() - xr.detach()).abs().max().item()
    e_sr = (sr.detach().cpu().double() - y.detach()).abs().max().item()
    gmax = max(v.grad.norm().item() for v in p.values() if v.grad is not None)
    worst, bad = 0.0, []
    for n, q in net.named_parameters():
        if n.startswith("stn_head"):
            continue
        ref = p[n].grad
        rel = (q.grad.cpu().double() - ref).norm().item() / max(ref.norm().item(), 1e-3 * gmax)
        worst = max(worst, rel)
        if rel > 2e-3:
            bad.append((n, rel))
    e_dprior = (pd.grad.cpu().double() - pr.grad).norm().item() / pr.grad.norm().item()
    dgrid = ws["stn_dgrid"].cpu().reshape(N, H, W, 2).double()
    e_dgrid = (dgrid - gl.grad).norm().item() / gl.grad.norm().item()
    print(f"x4 same grid: rectified err {e_xr:.2e}, SR err {e_sr:.2e}, loss {loss.item():.6f} vs {loss_ref.item():.6f}, worst non-STN "
          f"parameter-gradient rel err {worst:.2e}, dprior rel err {e_dprior:.2e}, grid-gradient rel err {e_dgrid:.2e}")
    assert e_xr < 2e-6 and e_sr < 5e-5
    assert abs(loss.item() - loss_ref.item()) < 1e-4 * abs(loss_ref.item())
    assert not bad, bad[:10]
    assert e_dprior < 2e-3
    assert e_dgrid < 2e-3
    # ---- stage A
    pa = X.params(sd)
    _, ctrl = O.stn_head(pa, "stn_head", lr64, True)
    ctrl.retain_grad()
    _, src = O.tps_transform(pa, "tps", lr64, ctrl, (H, W))
    grid_o = src.reshape(N, H, W, 2).clamp(0, 1) * 2.0 - 1.0
    assert (grid_o.detach() - grid_b).abs().max() < 2e-4          # (the two grids agree to the conditioning of the TPS system)
    grid_o.backward(gl.grad)
    e_dctrl = (ws["stn_dctrl"].cpu().reshape(N, 20, 2).double() - ctrl.grad).norm().item() / ctrl.grad.norm().item()
    gmax_a = max(v.grad.norm().item() for k, v in pa.items() if k.startswith("stn_head") and v.grad is not None)
    worst_a = 0.0
    for n, q in net.named_parameters():
        if n.startswith("stn_head"):
            ref = pa[n].grad
            rel = (q.grad.cpu().double() - ref).norm().item() / max(ref.norm().item(), 1e-3 * gmax_a)
            worst_a = max(worst_a, rel)
            assert rel < 2e-2 * NOISE, (n, rel)
    print(f"x4 same grid, STN head: control-point gradient rel err {e_dctrl:.2e}, worst head parameter-gradient rel err {worst_a:.2e}")
    assert e_dctrl < 5e-3


# ---- bicubic_gray at the x4 SR geometry ---------------------------------------------------------------------------------------------
def test_bicubic_gray_64x256_to_32x100_vs_float64():
    """parse_crnn_data's kernel pair from the x4 SR grid: a DOWN-sampling by 2 and 2.56 (until now ratios 1 and 1.28).  Forward and adjoint
    against float64 F.interpolate + luminance weights and its autograd, bound 4 e_ref32 + 4 * 2^-24 relative to max |ref| (tests/kernel_table.py);
    the mask plane gets exactly zero gradient; the adjoint is a gather (bitwise reproducible)."""
    from tpgsr_amd import kernels as K
    g = torch.Generator().manual_seed(64256)
    x = torch.rand(1, 4, 64, 256, generator=g)
    gy = torch.randn(1, 1, 32, 100, generator=g)
    res = {}
    for dt in (torch.float32, F64):
        xr = x.clone().to(dt).requires_grad_(True)
        y = O.parse_crnn_data(xr)
        y.backward(gy.to(dt))
        res[dt] = (y.detach().double(), xr.grad.double())
    out = torch.empty(1, 1, 32, 100, device=DEV)
    din, din2 = torch.full((1, 4, 64, 256), 7.0, device=DEV), torch.full((1, 4, 64, 256), -3.0, device=DEV)
    K.bicubic_gray_fwd(x.to(DEV), 1, 4, 64, 256, 32, 100, out)
    K.bicubic_gray_bwd(gy.to(DEV), 1, 4, 64, 256, 32, 100, din)
    K.bicubic_gray_bwd(gy.to(DEV), 1, 4, 64, 256, 32, 100, din2)
    torch.cuda.synchronize()
    for what, got, i in (("fwd", out, 0), ("bwd", din, 1)):
        r64, r32 = res[F64][i], res[torch.float32][i]
        scale = r64.abs().max().item()
        e_gpu, e32 = (got.cpu().double() - r64).abs().max().item() / scale, (r32 - r64).abs().max().item() / scale
        print(f"bicubic_gray {what} 64x256 -> 32x100: e_gpu {e_gpu:.2e}  e_ref32 {e32:.2e}")
        assert e_gpu <= 4 * e32 + 4 * 2.0 ** -24, (what, e_gpu, e32)
    assert float(din[:, 3].abs().max()) == 0.0 and float(res[F64][1][:, 3].abs().max()) == 0.0
    assert torch.equal(din, din2)


# ---- train steps --------------------------------------------------------------------------------------------------------------------
def test_x4_tsrn_train_step_two_steps_and_graph_replay():
    """TSRNTrainStep at x4 (N = 3, LR 5x18, no STN) against the restated float64 step: loss 2e-4 and clip norm 2e-3 at both steps
    (test_train_trajectory_nostn), last_sr 5e-5 at step 0 (test_three_channel_network_vs_oracle) and 5e-3 after an optimiser step
    (test_train_trajectory_nostn's final image); capture() / replay() bitwise the eager steps (test_train_step0_with_stn_and_graph_replay)"""
    from tpgsr_amd.interfaces.super_resolution import TSRNTrainStep
    from tpgsr_amd.model import tsrn
    _threads()
    kw = dict(scale_factor=4, width=256, height=64, STN=False, mask=True)
    sd = O.recipe_state_dict(O.tsrn_spec(srb_nums=5, **kw), 421)
    lr, hr = O.synthetic_batch(3, 422, lr_hw=(5, 18), scale=4)

    def build():
        net = tsrn.TSRN(**kw)
        net.load_state_dict(sd, strict=True)
        return net.to(DEV).train()

    net = build()
    ts = TSRNTrainStep(net)
    p = X.params(sd)
    opt = X.adam_for(p)
    lrd, hrd = lr.to(DEV), hr.to(DEV)
    for step in range(2):
        loss = ts.step(lrd, hrd)
        gn = ts.opt.grad_norm(net).item()
        ref = X.tsrn_train_step(p, opt, lr.double(), hr.double(), scale_factor=4, stn=False)
        e_sr = (ts.last_sr.cpu().double() - ref["sr"]).abs().max().item()
        print(f"x4 C2 step {step}: loss {loss.item():.6f} vs {ref['loss'].item():.6f}; clip norm {gn:.5f} vs {float(ref['grad_norm']):.5f}; last_sr err {e_sr:.2e}")
        assert tuple(ts.last_sr.shape) == (3, 4, 20, 72)
        assert abs(loss.item() - ref["loss"].item()) < 2e-4 * ref["loss"].item()
        assert abs(gn - float(ref["grad_norm"])) < 2e-3 * float(ref["grad_norm"])
        assert e_sr < (5e-5 if step == 0 else 5e-3)
    with pytest.raises(ValueError, match=r"\(N, C, 4H, 4W\)"):
        ts.step(lrd, F.avg_pool2d(hrd, 2))
    ta, tb = TSRNTrainStep(build()), TSRNTrainStep(build())
    tb.capture(lrd, hrd, warmup=1)
    la = [ta.step(lrd, hrd).item() for _ in range(3)]
    lb = [tb.replay().item() for _ in range(2)]
    torch.cuda.synchronize()
    print(la, lb)
    assert lb[0] == la[1] and lb[1] == la[2]
    assert torch.equal(ta.pool.flat, tb.pool.flat)


def _c3_models(sd_sr, sd_t, sd_s_list):
    from tpgsr_amd.model import tsrn
    from tpgsr_amd.model.crnn import crnn
    sr = tsrn.TSRN_TL(**X.X4_KW)
    sr.load_state_dict(sd_sr, strict=True)
    teacher = crnn.CRNN(32, 1, 37, 256)
    teacher.load_state_dict(sd_t)
    stus = []
    for sd in sd_s_list:
        s = crnn.CRNN(32, 1, 37, 256)
        s.load_state_dict(sd)
        stus.append(s.to(DEV).train())
    return sr.to(DEV).train(), stus, teacher.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _c3_reference():
    """the restated float64 cascade step on the fixture's case, two steps"""
    _threads()
    g, sd_sr, sd_t, sd_s, lr, hr = X.c3_fixture()
    ps, pt, pu = X.params(sd_sr), X.params(sd_t, False), X.params(sd_s)
    opt = X.adam_for(ps, pu)
    return [X.tpgsr_train_step([ps], [pu], pt, opt, lr.double(), hr.double(), scale_factor=4, stu_iter=1) for _ in range(2)]


def test_x4_tpgsr_train_step_vs_fixture_and_float64(golden_policy):
    """TPGSRTrainStep at x4 (N = 4, LR 16x64, STN) under x3 and x2.  Against the reference's numbers (train_c3_x4.npz), the bounds of
    test_crnn_gpu.py::test_train_c3_step_vs_golden: loss tol(3e-4), clip norm 3e-3, identical arg-max priors, step-1 loss 2e-2.  Against the
    restated float64 step, the bounds of test_fullsize_gpu.py::test_c3_bs48_step0_vs_oracle, flat under both policies: loss 3e-4, clip norm
    5e-3, priors 1e-5, and the
    two gates the project states, under both policies: |dPSNR| < 1e-3 dB and identical arg-max priors."""
    from tpgsr_amd.interfaces.super_resolution import TPGSRTrainStep
    g, sd_sr, sd_t, sd_s, lr, hr = X.c3_fixture()
    refs = _c3_reference()
    sr, stus, teacher = _c3_models(sd_sr, sd_t, [sd_s])
    ts = TPGSRTrainStep([sr], stus, teacher, stu_iter=1)
    assert ts.precision == golden_policy.name
    lrd, hrd = lr.to(DEV), hr.to(DEV)
    loss = ts.step(lrd, hrd)
    gn = ts.opt.grad_norm(sr).item()
    torch.cuda.synchronize()
    ref = refs[0]
    am = ts.last_p.cpu().permute(1, 0, 2).argmax(-1)
    dpsnr = abs(_psnr(ts.last_sr, hr) - _psnr(ref["sr"], hr))
    e_p = (ts.last_p.cpu().permute(1, 0, 2).double() - ref["priors"][0]).abs().max().item()
    e_lat = (ts.last_sr.cpu()[:, :, ::4, ::4] - torch.tensor(g["sr_step0_lattice"])).abs().max().item()
    print(f"x4 C3 step 0 {golden_policy.name}: loss {loss.item():.6f} vs fixture {g['loss'][0]:.6f} / float64 {ref['loss'].item():.6f}; clip norm {gn:.4f} vs "
          f"{g['gnorm'][0]:.4f} / {float(ref['grad_norms'][0]):.4f}; |dPSNR| {dpsnr:.2e} dB; prior err {e_p:.2e}; SR lattice vs fixture {e_lat:.2e}")
    assert tuple(ts.last_sr.shape) == (4, 4, 64, 256)
    assert abs(loss.item() - g["loss"][0]) < golden_policy.tol(3e-4) * g["loss"][0]
    assert abs(gn - g["gnorm"][0]) < 3e-3 * g["gnorm"][0]
    assert (am.numpy() == g["prior_argmax_step0"]).all()
    assert e_lat < 5e-3
    assert abs(loss.item() - ref["loss"].item()) < 3e-4 * ref["loss"].item()
    assert abs(gn - float(ref["grad_norms"][0])) < 5e-3 * float(ref["grad_norms"][0])
    assert dpsnr < 1e-3
    assert torch.equal(am, ref["priors"][0].argmax(-1))
    assert e_p < 1e-5
    l1 = ts.step(lrd, hrd).item()
    print(f"x4 C3 step 1 {golden_policy.name}: loss {l1:.6f} vs fixture {g['loss'][1]:.6f} / float64 {refs[1]['loss'].item():.6f}")
    assert abs(l1 - g["loss"][1]) < 2e-2 * g["loss"][1]
    assert abs(l1 - refs[1]["loss"].item()) < 2e-2 * refs[1]["loss"].item()


@functools.lru_cache(maxsize=None)
def _c3_share_reference():
    _threads()
    g, sd_sr, sd_t, sd_s, lr, hr = X.c3_fixture()
    sd_s2 = O.recipe_state_dict(O.crnn_spec(), int(g["student_seed"]) + 10)
    ps, pt, pu = X.params(sd_sr), X.params(sd_t, False), [X.params(sd_s), X.params(sd_s2)]
    return X.tpgsr_train_step([ps], pu, pt, X.adam_for(ps, *pu), lr.double(), hr.double(), scale_factor=4, stu_iter=2, sr_share=True), sd_s2


def test_x4_tpgsr_two_stages_sr_share_vs_float64(golden_policy):
    """stu_iter = 2, sr_share: stage 2 reads stage 1's 64x256 SR image through the 64x256 -> 32x100 resize and back-propagates through it.
    Bounds of test_fullsize_gpu.py::test_c5_shape_stu_iter3_sr_share_bs32_vs_oracle: loss 5e-4, clip norm 2e-2, |dPSNR| < 1e-3 dB,
    identical arg-max priors in every stage"""
    from tpgsr_amd.interfaces.super_resolution import TPGSRTrainStep
    g, sd_sr, sd_t, sd_s, lr, hr = X.c3_fixture()
    ref, sd_s2 = _c3_share_reference()
    sr, stus, teacher = _c3_models(sd_sr, sd_t, [sd_s, sd_s2])
    ts = TPGSRTrainStep([sr], stus, teacher, stu_iter=2, sr_share=True, tpg_share=False)
    loss = ts.step(lr.to(DEV), hr.to(DEV))
    gn = ts.opt.grad_norm(sr).item()
    torch.cuda.synchronize()
    dpsnr = abs(_psnr(ts.last_sr, hr) - _psnr(ref["sr"], hr))
    mism, margins = zip(*[X.argmax_mismatches(ts._static["p"][i].cpu().permute(1, 0, 2).double(), ref["priors"][i]) for i in range(2)])
    print(f"x4 two stages {golden_policy.name}: loss {loss.item():.6f} vs {ref['loss'].item():.6f}; clip norm {gn:.4f} vs {float(ref['grad_norms'][0]):.4f}; "
          f"|dPSNR| {dpsnr:.2e} dB; arg-max mismatches {mism} (oracle margins {margins})")
    assert abs(loss.item() - ref["loss"].item()) < 5e-4 * ref["loss"].item()
    assert abs(gn - float(ref["grad_norms"][0])) < 2e-2 * float(ref["grad_norms"][0])
    assert dpsnr < 1e-3
    assert list(mism) == [0, 0], (mism, margins)


def test_x4_train_step_bs48_default_policy_is_deterministic():
    """the x4 C3 step at its full size (bs 48, LR 16x64, STN) under the train steps' default policy x2, forward AND backward: two
    independent builds stepping the same batch three times end in bitwise the same losses and parameters (a missing stream edge or an
    index past a buffer at 786 432 SR pixels would show here; tests/test_tsrn_gpu.py::test_full_size_properties_bs48,
    test_crnn_gpu.py::test_train_c3_two_independent_runs_bitwise), the loss is finite and falls, SR stays inside the tanh range"""
    from tpgsr_amd.interfaces.super_resolution import TPGSRTrainStep
    g, sd_sr, sd_t, sd_s, _, _ = X.c3_fixture()
    lr, hr = O.synthetic_batch(48, 4850, scale=4)
    lrd, hrd = lr.to(DEV), hr.to(DEV)
    outs = []
    for _ in range(2):
        sr, stus, teacher = _c3_models(sd_sr, sd_t, [sd_s])
        ts = TPGSRTrainStep([sr], stus, teacher, stu_iter=1, precision="x2")
        assert ts.precision == "x2"
        losses = [ts.step(lrd, hrd).item() for _ in range(3)]
        torch.cuda.synchronize()
        assert tuple(ts.last_sr.shape) == (48, 4, 64, 256) and float(ts.last_sr.abs().max()) <= 1.0
        outs.append((losses, ts.pool.flat.clone()))
    print("x4 C3 bs48 x2 losses", outs[0][0])
    assert all(np.isfinite(v) for v in outs[0][0]) and outs[0][0][2] < outs[0][0][0]
    assert outs[0][0] == outs[1][0] and torch.equal(outs[0][1], outs[1][1])


# ---- evaluator ------------------------------------------------------------------------------------------------------------------------
def test_x4_evaluator_vs_float64():
    """TextSREvaluator.eval_batch at x4 (N = 4): SR 2e-5, PSNR 1e-3 dB, SSIM 1e-5, the recogniser's strings (tests/test_eval_gpu.py)"""
    from tpgsr_amd.interfaces.super_resolution import TextSREvaluator
    from tpgsr_amd.model.crnn import crnn
    _threads()
    g, sd_sr, sd_t, sd_s, lr, hr = X.c3_fixture()
    sr, stus, rec = _c3_models(sd_sr, sd_s, [sd_t])
    ev = TextSREvaluator([sr.eval()], [stus[0].eval()], rec, stu_iter=1)
    labels = ["abc", "7x", "", "hello"]
    out = ev.eval_batch(lr.to(DEV), hr.to(DEV), labels)
    torch.cuda.synchronize()
    ref = X.tpgsr_eval_step([X.params(sd_sr, False)], [X.params(sd_t, False)], X.params(sd_s, False), lr.double(), hr.double(),
                            scale_factor=4, stu_iter=1)
    e = (out["images_sr"][0].cpu().double() - ref["sr"][0]).abs().max().item()
    print(f"x4 eval: SR err {e:.2e}; psnr {float(out['psnr']):.5f} vs {float(ref['psnr']):.5f}; ssim {float(out['ssim']):.7f} vs {float(ref['ssim']):.7f}; "
          f"strings {out['pred_sr']} / {ref['pred_sr']}")
    assert tuple(out["images_sr"][0].shape) == (4, 4, 64, 256)
    assert e < 2e-5
    assert torch.equal(out["priors"][0].cpu().permute(1, 0, 2).argmax(-1), ref["priors"][0].argmax(-1))
    assert abs(float(out["psnr"]) - float(ref["psnr"])) < 1e-3
    assert abs(float(out["ssim"]) - float(ref["ssim"])) < 1e-5
    assert out["pred_sr"] == ref["pred_sr"] and out["pred_lr"] == ref["pred_lr"] and out["pred_hr"] == ref["pred_hr"]
    assert out["n_correct_sr"] == sum(a == b for a, b in zip(ref["pred_sr"], labels))


# ---- full size, once ------------------------------------------------------------------------------------------------------------------
def _fwd_routes(net):
    """(geometry, kernel, split-K plan) of every convolution of the eval plans recorded so far, per batch size"""
    from tpgsr_amd import kernels as K
    out = {}
    for key, pl in net._engine()._plans.items():
        for name, fn, args, sid in pl["pre"].ops + pl["fwd"].ops:
            if name == "tpgsr_conv_fwd":
                a = args[0]._obj
                kname, r = K.conv_route(a)
                out.setdefault(key[0], []).append((a.H, a.W, a.Cin, a.Cout, a.KH, a.KW, kname, r.sk_plan))
    return out


def test_x4_batch_independence_bs48():
    """bs 48, LR 16x64, eval mode (786 432 output pixels x 64 channels in the last up-sampling stage): rows 0, 23 and 47 of the batch equal
    the same images run alone, bitwise.  No float64 reference runs at this size.
    Bitwise equality across batch sizes needs every launch to reduce in the same order at N = 1 and N = 48, i.e. the same kernel and
    split-K plan per convolution: true for TSRN under the fp32-equivalent policy x3 (asserted below from the host-side route), not for
    TSRN_TL at any scale -- InfoGen's 512 -> 128 transposed convolution is split 8 ways at N = 1 and 4 ways at N = 48 -- so the
    text-prior network gets the size-preserving form of the property (test_full_size_properties_bs48): a permuted batch gives the
    permuted images, bitwise."""
    from tpgsr_amd import kernels as K
    from tpgsr_amd.model import tsrn
    prev = K.POLICY
    K.set_conv_prec("x3")
    try:
        kw = dict(scale_factor=4, width=256, height=64, STN=True, mask=True)
        net = tsrn.TSRN(**kw)
        net.load_state_dict(O.recipe_state_dict(O.tsrn_spec(srb_nums=5, **kw), 448, tps_hw=(16, 64)), strict=True)
        net = net.to(DEV).eval()
        lr, _ = O.synthetic_batch(48, 4848, scale=4)
        lrd = lr.to(DEV)
        with torch.no_grad():
            y = net(lrd)
            assert tuple(y.shape) == (48, 4, 64, 256) and float(y.abs().max()) <= 1.0 and bool(torch.isfinite(y).all())
            alone = {i: net(lrd[i:i + 1].contiguous()) for i in (0, 23, 47)}
        routes = _fwd_routes(net)
        assert [r[4:] for r in routes[1]] == [r[4:] for r in routes[48]]
        assert sum(r[2:4] == (64, 256) for r in routes[48]) == 2            # (both up-sampling convolutions are among them)
        for i, yi in alone.items():
            assert torch.equal(yi[0], y[i]), (i, (yi[0] - y[i]).abs().max().item())
        tl = _net("tl_stn").eval()
        pd = X.prior_from_seed(48, 4849).to(DEV)
        perm = torch.randperm(48, generator=torch.Generator().manual_seed(1)).to(DEV)
        with torch.no_grad():
            z = tl(lrd, pd)
            zp = tl(lrd[perm].contiguous(), pd[perm].contiguous())
        assert tuple(z.shape) == (48, 4, 64, 256) and torch.equal(zp, z[perm])
    finally:
        K.set_conv_prec(prev)
