"""GPU: the `_TL` baseline backbones (SRResNet_TL / SRCNN_TL / VDSR_TL / RDN_TL) as the SR network of the fused cascade step
(`TPGSRTrainStep`, reference interfaces/super_resolution.py:295-424 with `--arch srresnet_tl | srcnn_tl | vdsr_tl | rdn_tl`) through
engine_functional.FunctionalSREngine: against fixtures composed from the reference's own modules (tests/golden/make_golden_tl_cascade.py),
recorded plans against the operator-by-operator run on fresh inputs, the two-slot cascade, hipGraph capture, the n-way gradient sum
tpgsr_add_n, the L1 criterion's kernels against float64, and the evaluator."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from kernel_table import KCase, _gen, check_case  # noqa: E402
from make_golden_next import generic_recipe  # noqa: E402  (the weight recipe only; the reference is not imported here)
from make_golden_tl_cascade import BACKBONES, CRIT, SEEDS  # noqa: E402  (names, criteria and seeds only)
from oracle import tpgsr_oracle as O  # noqa: E402

DEV = "cuda"
N = 4


def build_backbone(name):
    from tpgsr_amd.model import rdn, srcnn, srresnet, vdsr
    if name == "srresnet_tl":
        return srresnet.SRResNet_TL(scale_factor=2, width=128, height=32, STN=False, mask=True)
    if name == "srcnn_tl":
        return srcnn.SRCNN_TL(scale_factor=2, width=128, height=32, STN=False)
    if name == "vdsr_tl":
        return vdsr.VDSR_TL(scale_factor=2, width=128, height=32, STN=False)
    return rdn.RDN_TL(scale_factor=2)


def build(name, stu_iter=1):
    """SR net, students, teacher on the GPU with the fixture's recipe weights, and the fixture's batch"""
    from tpgsr_amd.model.crnn import crnn
    dseed, wseed, tseed, sseeds = SEEDS[name]
    net = build_backbone(name)
    net.load_state_dict(generic_recipe(net.state_dict(), wseed))
    teacher = crnn.CRNN(32, 1, 37, 256)
    teacher.load_state_dict(O.recipe_state_dict(O.crnn_spec(), tseed))
    stus = []
    for i in range(stu_iter):
        s = crnn.CRNN(32, 1, 37, 256)
        s.load_state_dict(O.recipe_state_dict(O.crnn_spec(), sseeds[i]))
        stus.append(s.to(DEV).train())
    lr, hr = O.synthetic_batch(N, dseed)
    return net.to(DEV).train(), stus, teacher.to(DEV).eval(), lr.to(DEV), hr.to(DEV)


def make_step(name, net, stus, teacher, stu_iter=1, precision="x3"):
    from tpgsr_amd.interfaces.super_resolution import TPGSRTrainStep
    return TPGSRTrainStep([net], stus, teacher, stu_iter=stu_iter, sr_share=True, tpg_share=False, image_crit=CRIT[name], precision=precision)


def check_param_grads(tag, module, names, norms, heads):
    """every parameter gradient: norm and leading entries with the rule and bounds of tests/test_next_models_gpu.py (5e-3; 2e-2 for
    one-element tensors)"""
    P = dict(module.named_parameters())
    gmax = norms.max()
    worst = 0.0
    for n, ref_norm, head in zip([str(n) for n in names], norms, heads):
        got = P[n].grad.detach().cpu()
        en = abs(got.double().norm().item() - ref_norm) / max(ref_norm, 1e-3 * gmax)
        k = min(8, got.numel())
        sc = max(ref_norm / np.sqrt(got.numel()), 1e-3 * gmax / np.sqrt(got.numel()))
        eh = (got.reshape(-1)[:k] - torch.tensor(head[:k])).abs().max().item() / sc
        worst = max(worst, en)
        tol = 2e-2 if got.numel() == 1 else 5e-3
        assert en < tol and eh < 0.1 * (tol / 5e-3), (tag, n, en, eh)
    print(f"   {tag}: worst parameter-gradient norm rel err {worst:.2e}")


def global_grad_err(module, names, norms):
    """relative error of the global gradient norm composed from the per-parameter norms"""
    P = dict(module.named_parameters())
    got = np.array([P[str(n)].grad.double().norm().item() for n in names])
    return float(np.sqrt(((got - norms) ** 2).sum() / (norms ** 2).sum()))


def run_against_fixture(name, golden_dir, stu_iter, fixture):
    t = np.load(os.path.join(golden_dir, fixture))
    net, stus, teacher, lr, hr = build(name, stu_iter)
    from tpgsr_amd import kernels as K
    ts = make_step(name, net, stus, teacher, stu_iter)
    # raw gradients of step 0 (before the clip), then the two optimiser steps from the same initial state
    ts.pool.bind(torch.device(DEV, 0))
    teacher._engine().bind(torch.device(DEV, 0))
    with K.policy(ts.precision):
        ts._phase_a(lr, hr)
    torch.cuda.synchronize()
    check_param_grads(name, net, t["sr_grad_names"], t["sr_grad_norms"], t["sr_grad_heads"])
    for i, s in enumerate(stus):
        e = global_grad_err(s, t[f"stu{i}_grad_names"], t[f"stu{i}_grad_norms"])
        print(f"   {name}: student {i} global gradient rel err {e:.2e}")
        assert e < 2e-2
    # BatchNorm statistics moved in that pass: the two optimiser steps start from the recipe again
    net2, stus2, teacher2, _, _ = build(name, stu_iter)
    ts = make_step(name, net2, stus2, teacher2, stu_iter)
    losses, gns = [], []
    for step in range(2):
        loss = ts.step(lr, hr)
        torch.cuda.synchronize()
        losses.append(loss.item())
        gns.append(ts.opt.grad_norm(net2).item())
        if step == 0 and "sr_step0" in t.files:
            assert (ts.last_p.cpu().permute(1, 0, 2).argmax(-1).numpy() == t["prior_argmax_step0"]).all()
            ref = torch.tensor(t["sr_step0"])
            e = (ts.last_sr.cpu() - ref).abs().max().item()
            print(f"   {name}: sr_step0 max err {e:.2e}")
            assert e < 1e-4 * max(1.0, float(ref.abs().max()))
    print(f"{name} (stu_iter {stu_iter}) losses {losses} vs {t['loss']}; SR clip norms {gns} vs {t['gnorm']}")
    assert abs(losses[0] - t["loss"][0]) < 3e-4 * t["loss"][0]
    assert abs(gns[0] - t["gnorm"][0]) < 3e-3 * t["gnorm"][0]
    assert abs(losses[1] - t["loss"][1]) < 2e-2 * t["loss"][1]
    return ts


# ---- 1. per backbone against its fixture (x3) --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BACKBONES)
def test_tl_backbone_cascade_step_vs_reference_fixture(name, golden_dir):
    ts = run_against_fixture(name, golden_dir, 1, f"train_tl_{name}.npz")
    net, stu = ts.sr[0], ts.stu[0]
    from tpgsr_amd.engine_functional import FunctionalSREngine
    assert isinstance(net._engine(), FunctionalSREngine) and net._engine().record
    for m in (net, stu):      # SR net and student live in the pooled arena
        a, b = ts.pool.ranges[id(m)]
        assert ts.pool.flat[a:b].data_ptr() == m._engine().arena.flat.data_ptr()


@pytest.mark.parametrize("name", BACKBONES)
def test_tl_backbone_two_term_policy_holds_the_gates(name, golden_dir):
    """the step's default policy x2 with these backbones, against the same reference fixture, with the bounds tests/test_policy_x2_gpu.py
    sets for TSRN_TL: |dPSNR| < 1e-3 dB, identical arg-max priors, loss within 2e-5, SR gradient norm within 2e-3"""
    t = np.load(os.path.join(golden_dir, f"train_tl_{name}.npz"))
    net, stus, teacher, lr, hr = build(name)
    ts = make_step(name, net, stus, teacher, precision="x2")
    loss = ts.step(lr, hr).item()
    torch.cuda.synchronize()
    gn = ts.opt.grad_norm(net).item()
    ref = torch.tensor(t["sr_step0"])
    dpsnr = abs(float(O.calculate_psnr(ts.last_sr.cpu(), hr.cpu())) - float(O.calculate_psnr(ref, hr.cpu())))
    mism = int((ts.last_p.cpu().permute(1, 0, 2).argmax(-1).numpy() != t["prior_argmax_step0"]).sum())
    print(f"{name} x2: loss {loss:.6f} vs {t['loss'][0]:.6f}; |dPSNR| {dpsnr:.3e} dB; arg-max mismatches {mism}; SR clip norm {gn:.5f} vs {t['gnorm'][0]:.5f}")
    assert dpsnr < 1e-3
    assert mism == 0
    assert abs(loss - t["loss"][0]) < 2e-5 * t["loss"][0]
    assert abs(gn - t["gnorm"][0]) < 2e-3 * t["gnorm"][0]


# ---- 2. recorded against operator by operator, on inputs other than the traced ones ---------------------------------------------------
def _passes(name, record, n_pass=3):
    from tpgsr_amd import kernels as K
    net = build_backbone(name)
    net.load_state_dict(generic_recipe(net.state_dict(), SEEDS[name][1]))
    net = net.to(DEV).train()
    eng = net._engine()
    eng.record = record
    g = torch.Generator().manual_seed(91)
    outs = []
    with K.policy("x3"):
        for i in range(n_pass):
            lr = torch.rand(N, 4, 16, 64, generator=g).to(DEV)
            prior = torch.softmax(torch.randn(N, 37, 1, 26, generator=g) * 2, 1).to(DEV)
            dsr = torch.randn(N, 4, 32, 128, generator=g).to(DEV)
            sr = eng.forward(lr, True, prior, slot=i % 2)
            eng.arena.attach_grads()
            eng.arena.grad.zero_()
            dprior = eng.backward(tuple(lr.shape), sr, dsr, slot=i % 2)
            torch.cuda.synchronize()
            outs.append(dict(sr=sr.clone(), dprior=dprior.clone(), grad=eng.arena.grad.clone()))
    eng.flush_counters()
    return outs, {k: v.clone() for k, v in net.named_buffers()}, eng


@pytest.mark.parametrize("name", BACKBONES)
def test_recorded_plan_equals_operator_by_operator_run(name):
    rec, bufs_r, eng = _passes(name, True)
    ref, bufs_e, _ = _passes(name, False)
    assert len(eng._plans) == 2 and all(len(pl["fwd"]) > 20 and len(pl["bwd"]) > 20 for pl in eng._plans.values())
    for i, (a, b) in enumerate(zip(rec, ref)):
        assert torch.equal(a["sr"], b["sr"]), (i, float((a["sr"] - b["sr"]).abs().max()))
        assert torch.equal(a["dprior"], b["dprior"]), (i, float((a["dprior"] - b["dprior"]).abs().max()))
        d = (a["grad"] - b["grad"]).abs().max().item()
        assert d <= 1e-6 * b["grad"].abs().max().item(), (i, d)
    assert bufs_e
    for k in bufs_e:
        assert torch.equal(bufs_r[k].float(), bufs_e[k].float()), k


# ---- 3. two slots: shared SR net, a student per stage, gradient through parse_crnn_data into the previous SR image ----------------------
def test_two_slot_cascade_vs_reference_fixture(golden_dir):
    run_against_fixture("srresnet_tl", golden_dir, 2, "train_tl_srresnet_tl_s2.npz")


# ---- 4. capture + replay -----------------------------------------------------------------------------------------------------------
def test_capture_replay_equals_eager_steps():
    """capture() applies one eager warm-up step and executes nothing itself: two replays are bitwise the eager twin's second and third step
    (recorded plans inside a hipGraph: same kernels, same order, deterministic reductions)"""
    name = "srresnet_tl"
    net_a, stus_a, teacher_a, lr, hr = build(name)
    net_b, stus_b, teacher_b, _, _ = build(name)
    ea, eb = make_step(name, net_a, stus_a, teacher_a), make_step(name, net_b, stus_b, teacher_b)
    eb.capture(lr, hr, warmup=1)
    la = [ea.step(lr, hr).item() for _ in range(3)]
    lb = [eb.replay().item() for _ in range(2)]
    torch.cuda.synchronize()
    print(la, lb)
    assert lb[0] == la[1] and lb[1] == la[2]
    assert torch.equal(ea.pool.flat, eb.pool.flat)
    assert torch.equal(ea.last_sr, eb.last_sr)


# ---- 5. tpgsr_add_n -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(2, 9))
def test_add_n_is_the_left_to_right_fp32_sum(k):
    from tpgsr_amd import kernels as K
    g = torch.Generator().manual_seed(100 + k)
    for n in (1, 3, 4 * 37 + 1, 4096 * 256 * 4 + 4 * 11 + 1):       # the last: above the span of one pass of the largest grid
        xs = [torch.randn(n, generator=g) * 10.0 ** float(torch.randint(-3, 4, (1,), generator=g)) for _ in range(k)]
        want = xs[0].clone()
        for x in xs[1:]:
            want = want + x
        out = torch.full((n,), float("nan"), device=DEV)
        K.add_n([x.to(DEV) for x in xs], n, out)
        assert torch.equal(out.cpu(), want), (k, n)
        if n > 8:      # unaligned addends take the element-by-element path: same bits
            big = [torch.cat([torch.zeros(1), x]).to(DEV)[1:] for x in xs]
            out2 = torch.full((n,), float("nan"), device=DEV)
            K.add_n(big, n, out2)
            assert torch.equal(out2.cpu(), want), (k, n, "unaligned")


@pytest.mark.parametrize("n", [3, 5, 8])
def test_fork_n_sums_the_gradients_of_its_consumers(n):
    from tpgsr_amd import functional as Fh
    g = torch.Generator().manual_seed(n)
    x = torch.randn(2, 3, 5, 4, generator=g).to(DEV).requires_grad_(True)
    ws = [torch.randn(2, 3, 5, 4, generator=g).to(DEV) for _ in range(n)]
    for used in (list(range(n)), [n - 2], [0] + list(range(2, n))):      # all consumers; all but one unused; one unused
        x.grad = None
        views = Fh.fork(x, n)
        assert len(views) == n and all(torch.equal(v, x) for v in views)
        sum((views[i] * ws[i]).sum() for i in used).backward()
        want = ws[used[0]].clone()
        for i in used[1:]:
            want = want + ws[i]
        assert torch.equal(x.grad, want), used
    with pytest.raises(ValueError):
        Fh.fork(x, 9)


# ---- 6. the L1 criterion's kernels against float64 (the rule of tests/kernel_table.py) --------------------------------------------------
def _l1_make(shape, seed):
    g = _gen("l1_loss", shape, seed)
    tgt = torch.rand(*shape, generator=g)
    out = tgt + 0.3 * torch.randn(*shape, generator=g)
    same = torch.rand(*shape, generator=g) < 0.1       # every tenth element: sr == hr exactly, gradient 0
    same.reshape(-1)[0] = True
    out = torch.where(same, tgt, out)
    return {"out": out, "tgt": tgt, "dl": torch.rand(1, generator=g) + 0.5}


def _l1_ref(d, w):
    out = d["out"].clone().requires_grad_(True)
    loss = F.l1_loss(out, d["tgt"]) * w
    (loss * d["dl"][0]).backward()
    return {"loss": loss.detach().reshape(()), "dout": out.grad}


def _l1_gpu(d, w, nblk):
    from tpgsr_amd import kernels as K
    out, tgt = d["out"], d["tgt"]
    part = torch.full((nblk, 2), float("nan"), device=DEV)
    loss = torch.full((1,), float("nan"), device=DEV)
    dout = torch.full_like(out, float("nan"))
    K.l1_loss_fwd(out, tgt, out.numel(), part, nblk)
    K.image_loss_finalize(part, nblk, out.numel(), 0, w, 0.0, loss)
    K.l1_loss_bwd(out, tgt, d["dl"], out.numel(), w, dout)
    return {"loss": loss.reshape(()), "dout": dout}


L1_CASES = [KCase("l1_loss", f"{'x'.join(map(str, shape))}-w{w:g}-nblk{nblk}", lambda seed, shape=shape: _l1_make(shape, seed),
                  lambda d, w=w: _l1_ref(d, w), lambda d, w=w, nblk=nblk: _l1_gpu(d, w, nblk), scalars=["loss"])
            for shape in [(2, 4, 3, 5), (1, 3, 32, 128)] for w, nblk in [(100.0, 1024), (1.0, 3)]]


@pytest.mark.parametrize("case", L1_CASES, ids=[c.id for c in L1_CASES])
def test_l1_loss_kernels_vs_float64(case):
    same = case.ins["out"] == case.ins["tgt"]
    assert same.any() and not same.all()
    check_case(case, {})
    from kernel_table import run_gpu
    assert (run_gpu(case)["dout"][same] == 0).all()         # sign(0) = 0, as ATen's L1 backward


# ---- 7. evaluator --------------------------------------------------------------------------------------------------------------------
def test_evaluator_with_a_tl_backbone():
    from tpgsr_amd.interfaces.super_resolution import TextSREvaluator, TPGSRTrainStep
    name = "srresnet_tl"
    net, stus, teacher, lr, hr = build(name)
    ts = make_step(name, net, stus, teacher)
    ts.step(lr, hr)
    net.eval(), stus[0].eval()
    ev = TextSREvaluator([net], stus, stu_iter=1)
    srs, priors = ev.super_resolve(lr)
    prior = priors[0].permute(0, 2, 1).reshape(N, 37, 1, 26).contiguous()      # (N, 26, 37) -> (N, 37, 1, 26)
    with torch.no_grad():
        want = net(lr, prior)
    torch.cuda.synchronize()
    assert torch.equal(srs[0], want), float((srs[0] - want).abs().max())
    for m in (net, stus[0]):
        a, b = ts.pool.ranges[id(m)]
        assert ts.pool.flat[a:b].data_ptr() == m._engine().arena.flat.data_ptr()
        lo, hi = ts.pool.flat.data_ptr(), ts.pool.flat.data_ptr() + 4 * ts.pool.flat.numel()
        assert all(lo <= p.data_ptr() < hi for p in m.parameters())
