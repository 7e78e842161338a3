"""GPU: TSRN / TSRN_TL with hidden_units = 64 (a 128-channel trunk, 64-unit BiGRUs: the reference's `--hd_u 64`) against the oracle and
against the reference-pinned fixture tests/golden/model_tsrn_tl_hd64.npz.  Every tolerance is the one tests/test_tsrn_gpu.py /
tests/test_crnn_gpu.py assert for hidden_units = 32 on the same quantity; the line is cited next to each."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import tpgsr_oracle as O  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_hd64_cpu import hd64_fixture  # noqa: E402

DEV = "cuda"
NOISE = 1.5      # tests/test_tsrn_gpu.py:18 (the STN head's discontinuous gradients)
HD = 64


def _build(tl, stn, srb, seed):
    from tpgsr_amd.model import tsrn
    sd = O.recipe_state_dict(O.tsrn_spec(STN=stn, mask=True, text_prior=tl, srb_nums=srb, hidden_units=HD), seed, tps_hw=(16, 64))
    net = (tsrn.TSRN_TL if tl else tsrn.TSRN)(STN=stn, mask=True, srb_nums=srb, hidden_units=HD)
    net.load_state_dict(sd, strict=True)
    return net.to(DEV), sd


def _prior(n, seed):
    return torch.softmax(torch.randn(n, 37, 1, 26, generator=torch.Generator().manual_seed(seed)) * 2, 1)


@pytest.mark.parametrize("tl", [False, True])
def test_hd64_nostn_vs_oracle(tl):
    """no STN, srb_nums 2, N = 2, LR 8 x 16: eval forward, train forward + ImageLoss, every parameter gradient element-wise, BN buffers"""
    from tpgsr_amd.loss.image_loss import ImageLoss
    net, sd = _build(tl, False, 2, 31)
    lr, hr = O.synthetic_batch(2, 8, lr_hw=(8, 16))
    prior = (_prior(2, 5),) if tl else ()
    kw = dict(stn=False, srb_nums=2, text_prior=tl)
    with torch.no_grad():
        y_eval = O.tsrn_forward(O.as_params(sd, False), lr, *prior, training=False, **kw)
    net.eval()
    with torch.no_grad():
        e = (net(lr.to(DEV), *[q.to(DEV) for q in prior]).cpu() - y_eval).abs().max().item()
    print("eval forward max err", e)
    assert e < 5e-5                                                           # tests/test_tsrn_gpu.py:74 (x3)
    p = O.as_params(sd)
    y = O.tsrn_forward(p, lr, *prior, training=True, **kw)
    loss_ref = O.image_loss(y, hr).mean() * 100
    loss_ref.backward()
    net.train()
    sr = net(lr.to(DEV), *[q.to(DEV) for q in prior])
    loss = ImageLoss(gradient=True, loss_weight=[1, 1e-4])(sr, hr.to(DEV)).mean() * 100
    loss.backward()
    assert (sr.detach().cpu() - y.detach()).abs().max() < 5e-5               # tests/test_tsrn_gpu.py:91 / :326
    assert abs(loss.item() - loss_ref.item()) < 1e-4 * abs(loss_ref.item())  # tests/test_tsrn_gpu.py:92
    gmax = max(v.grad.norm().item() for v in p.values() if v.grad is not None)
    bad, worst = [], 0.0
    for n, q in net.named_parameters():
        ref = p[n].grad
        rel = (q.grad.cpu() - ref).norm().item() / max(ref.norm().item(), 1e-3 * gmax)
        worst = max(worst, rel)
        if rel > 2e-3:                                                        # tests/test_tsrn_gpu.py:332 (test_tsrn_tl_gradients_vs_oracle_nostn)
            bad.append((n, rel))
    print("worst relative gradient error", worst)
    assert not bad, bad[:10]
    B = dict(net.named_buffers())
    for k, v in p.items():
        if "running_" in k:
            assert (B[k].cpu() - v.detach()).abs().max() < 2e-4, k            # tests/test_tsrn_gpu.py:66


def test_hd64_with_stn_vs_oracle(golden_policy):
    """STN on (the head only takes 16 x 64), srb_nums 1, N = 2: loss and gradient norm as test_three_channel_network_vs_oracle with STN"""
    from tpgsr_amd.interfaces.super_resolution import TSRNTrainStep
    net, sd = _build(False, True, 1, 32)
    lr, hr = O.synthetic_batch(2, 9)
    p = O.as_params(sd)
    y = O.tsrn_forward(p, lr, training=True, stn=True, srb_nums=1)
    loss_ref = O.image_loss(y, hr).mean() * 100
    loss_ref.backward()
    gref = torch.sqrt(sum((v.grad.double() ** 2).sum() for v in p.values() if v.grad is not None)).item()
    net.train()
    ts = TSRNTrainStep(net)
    loss = ts.step(lr.to(DEV), hr.to(DEV))
    gn = ts.opt.grad_norm(net).item()
    print(f"{golden_policy.name}: loss {loss.item():.6f} (oracle {loss_ref.item():.6f}), gradient norm {gn:.4f} (oracle {gref:.4f})")
    assert abs(loss.item() - loss_ref.item()) < golden_policy.tol(3e-4) * abs(loss_ref.item())      # tests/test_tsrn_gpu.py:396
    assert abs(gn - gref) < 2e-2 * NOISE * gref                                                       # tests/test_tsrn_gpu.py:397


def test_hd64_train_trajectory_nostn():
    """TSRNTrainStep, two steps, against the oracle's loss / clipped-gradient norm per step: 2e-4 / 2e-3 (test_train_trajectory_nostn)"""
    from tpgsr_amd.interfaces.super_resolution import TSRNTrainStep
    net, sd = _build(False, False, 2, 33)
    lr, hr = O.synthetic_batch(2, 10, lr_hw=(8, 16))
    p = O.as_params(sd)
    opt = O.AdamState([p[k] for k in O.trainable_keys(p)])
    net.train()
    ts = TSRNTrainStep(net)
    for step in range(2):
        r = O.tsrn_train_step(p, opt, lr, hr, stn=False, srb_nums=2)
        loss = ts.step(lr.to(DEV), hr.to(DEV))
        gn = ts.opt.grad_norm(net).item()
        print(step, loss.item(), float(r["loss"]), gn, float(r["grad_norm"]))
        assert abs(loss.item() - float(r["loss"])) < 2e-4 * float(r["loss"])                # tests/test_tsrn_gpu.py:116
        assert abs(gn - float(r["grad_norm"])) < 2e-3 * float(r["grad_norm"])               # tests/test_tsrn_gpu.py:117


def _c3(seed=300):
    from tpgsr_amd.model.crnn import crnn
    sr, sd_sr = _build(True, True, 2, seed + 1)
    sd_t, sd_s = O.recipe_state_dict(O.crnn_spec(), seed + 2), O.recipe_state_dict(O.crnn_spec(), seed + 3)
    teacher, stu = crnn.CRNN(32, 1, 37, 256), crnn.CRNN(32, 1, 37, 256)
    teacher.load_state_dict(sd_t)
    stu.load_state_dict(sd_s)
    return sr.train(), stu.to(DEV).train(), teacher.to(DEV).eval(), sd_sr, sd_s, sd_t


@pytest.mark.parametrize("policy", ["x3", "x2"])
def test_hd64_tpgsr_step_vs_oracle(policy):
    """one TPGSRTrainStep([TSRN_TL(hidden_units=64, srb_nums=2)], [CRNN], CRNN) step at N = 4 under both arithmetic policies: loss against
    the oracle, identical arg-max priors, |dPSNR| < 1e-3 dB (the gates of smoke() / tests/test_crnn_gpu.py:278-280)"""
    from tpgsr_amd.interfaces.super_resolution import TPGSRTrainStep
    sr, stu, teacher, sd_sr, sd_s, sd_t = _c3()
    lr, hr = O.synthetic_batch(4, 12)
    ts = TPGSRTrainStep([sr], [stu], teacher, stu_iter=1, precision=policy)
    loss = ts.step(lr.to(DEV), hr.to(DEV))
    torch.cuda.synchronize()
    ps, pt, pu = O.as_params(sd_sr), O.as_params(sd_t, False), O.as_params(sd_s)
    opt = O.AdamState([ps[k] for k in O.trainable_keys(ps)] + [pu[k] for k in O.trainable_keys(pu)])
    ref = O.tpgsr_train_step([ps], [pu], pt, opt, lr, hr, stu_iter=1, srb_nums=2)
    err = abs(loss.item() - ref["loss"].item()) / abs(ref["loss"].item())
    gn, gref = ts.opt.grad_norm(sr).item(), float(ref["grad_norms"][0])
    dpsnr = abs(float(O.calculate_psnr(ts.last_sr.cpu(), hr)) - float(O.calculate_psnr(ref["sr"], hr)))
    print(f"{policy}: loss rel err {err:.2e}, SR grad norm {gn:.4f} (oracle {gref:.4f}), |dPSNR| {dpsnr:.2e} dB")
    assert err < (3e-4 if policy == "x3" else 8 * 3e-4)                      # tests/test_crnn_gpu.py:278 (golden_policy.tol(3e-4))
    assert torch.equal(ts.last_p.cpu().permute(1, 0, 2).argmax(-1), ref["priors"][0].argmax(-1))
    assert dpsnr < 1e-3


def test_hd64_tpgsr_graph_replay_equals_eager():
    """the captured step replayed == the eager step sequence, bitwise (tests/test_crnn_gpu.py::test_train_c3_hipgraph_replay_equals_eager);
    the replay runs on a SECOND input"""
    from tpgsr_amd.interfaces.super_resolution import TPGSRTrainStep
    lr, hr = (t.to(DEV) for t in O.synthetic_batch(4, 12))
    lr2, hr2 = (t.to(DEV) for t in O.synthetic_batch(4, 13))
    (sa, ua, ta, *_), (sb, ub, tb, *_) = _c3(), _c3()
    ea, eb = TPGSRTrainStep([sa], [ua], ta, stu_iter=1), TPGSRTrainStep([sb], [ub], tb, stu_iter=1)
    eb.capture(lr, hr, warmup=1)
    la = [ea.step(lr, hr).item(), ea.step(lr2, hr2).item()]
    lb = eb.replay(lr2, hr2).item()
    torch.cuda.synchronize()
    assert lb == la[1]
    assert torch.equal(ea.pool.flat, eb.pool.flat)


def test_hd64_evaluator_equals_module_eval_forward():
    from tpgsr_amd.interfaces.super_resolution import TextSREvaluator
    sr, stu, teacher, *_ = _c3()
    sr.eval()
    stu.eval()
    lr, _ = O.synthetic_batch(3, 14)
    ev = TextSREvaluator([sr], [stu], teacher, stu_iter=1)
    srs, priors = ev.super_resolve(lr.to(DEV))
    with torch.no_grad():
        y = sr(lr.to(DEV), priors[0].permute(0, 2, 1).unsqueeze(2).contiguous())
    torch.cuda.synchronize()
    assert tuple(y.shape) == (3, 4, 32, 128) and torch.equal(srs[0], y)


def test_hd64_vs_reference_fixture(golden_policy):
    """the reference's own TSRN_TL(hidden_units=64) numbers (tests/golden/make_golden_hd64.py): SR image, loss, per-parameter gradient norms,
    with the bounds of test_tsrn_tl_vs_golden"""
    from tpgsr_amd.loss.image_loss import ImageLoss
    from tpgsr_amd.model import tsrn
    g, sd, lr, hr, prior = hd64_fixture()
    lr, hr, prior = lr.to(DEV), hr.to(DEV), prior.to(DEV)

    def build():
        net = tsrn.TSRN_TL(STN=True, mask=True, hidden_units=HD)
        net.load_state_dict(sd, strict=True)
        return net.to(DEV)

    net = build().train()
    sr = net(lr, prior)
    err = (sr.detach().cpu() - torch.tensor(g["sr_train"])).abs().max().item()
    print("train forward max err", err)
    assert err < 5e-3                                                                           # tests/test_tsrn_gpu.py:291
    loss = ImageLoss(gradient=True, loss_weight=[1, 1e-4])(sr, hr).mean() * 100
    assert abs(loss.item() - float(g["loss"])) < golden_policy.tol(3e-4) * float(g["loss"])     # tests/test_tsrn_gpu.py:293
    loss.backward()
    P = dict(net.named_parameters())
    gmax = g["grad_norms"].max()
    for n, ref_norm in zip(json.loads(str(g["grad_names"])), g["grad_norms"]):
        e = abs(P[n].grad.double().norm().item() - ref_norm) / max(ref_norm, 1e-3 * gmax)
        assert e < 2e-2, (n, e, ref_norm)                                                       # tests/test_tsrn_gpu.py:299
    net2 = build().eval()
    with torch.no_grad():
        y = net2(lr, prior)
    err = (y.cpu() - torch.tensor(g["sr_eval"])).abs().max().item()
    print("eval forward max err", err, golden_policy.name)
    assert err < golden_policy.tol(5e-5)                                                        # tests/test_tsrn_gpu.py:306
