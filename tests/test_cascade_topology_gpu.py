"""GPU: the multi-stage cascade with the reference's default topology -- one SR network per stage (`--sr_share` off, main.py:44-45;
model_list, interfaces/super_resolution.py:90-94 / :354-358, each clipped on its own at :421-422) -- and with one text-prior generator
shared by every stage (`--tpg_share`, :307-311).  Per-stage SR nets are three arenas in the pooled buffer, three clip groups in FusedAdam
and three re-packs after Adam; a shared student runs three training forwards and three backward passes per step through slots 0..2, all
ACCUMULATING into one gradient arena, and its BatchNorm running statistics move three times.

  * against the reference's own numbers (tests/golden/train_cascade_topologies.npz, make_golden_cascade.py), x3 and x2;
  * full size (bs 32, stu_iter 3, STN) against the oracle: loss, PSNR, priors, three clip norms, running statistics, determinism;
  * raw gradients (no optimiser) against the oracle in fp64;
  * three-stream schedule == serial schedule, hipGraph replay == eager, for the shared student."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import tpgsr_oracle as O  # noqa: E402
from test_crnn_gpu import _c3_models  # noqa: E402
from test_fullsize_gpu import _psnr, _threads, argmax_mismatches  # noqa: E402
from test_oracle_golden import cascade_models  # noqa: E402
from test_schedule_gpu import _reset, _run, schedule  # noqa: E402,F401  (fixture)

DEV = "cuda"
S = 3
LAYOUTS = {"a": (False, False), "b": (False, True), "c": (True, True)}     # sr_share, tpg_share
BETA1 = 0.5


def _step(layout, seeds, stn=True):
    from tpgsr_amd.interfaces.super_resolution import TPGSRTrainStep
    sr_share, tpg_share = LAYOUTS[layout]
    srs, stus, teacher, sds, sd_s, sd_t = _c3_models(seeds=seeds, stn=stn, n_sr=1 if sr_share else S, n_stu=1 if tpg_share else S)
    ts = TPGSRTrainStep(srs, stus, teacher, stu_iter=S, sr_share=sr_share, tpg_share=tpg_share)
    return ts, srs, stus, sds, sd_s, sd_t


def _clipped_moment_norms(ts, srs, norms):
    """after ONE step every SR net's Adam first moment is (1 - beta1) * its OWN clipped gradient: |m| = (1 - beta1) * min(norm, 0.25)
    up to rounding.  (Adam's first update is ~ lr * sign(g) whatever the scale, so the clip coefficient shows here, not in the loss.)"""
    out = []
    for m, n in zip(srs, norms):
        st = ts.opt.state[id(m)]
        got = st["m"].double().norm().item()
        want = (1 - BETA1) * min(1.0, 0.25 / (n + 1e-6)) * n
        out.append(abs(got - want) / max(want, 1e-30))
    return out


@pytest.mark.parametrize("layout", ["a", "b", "c"])
def test_cascade_topology_vs_reference_fixture(golden_dir, golden_policy, layout):
    """stu_iter 3, N 4, STN on, layouts a (three SR nets, three students), b (three SR nets, one shared student), c (one of each):
    step-0 loss, EVERY SR net's clip norm on its own, every stage's arg-max prior, and step 1 -- the first forward after Adam rewrote
    each of the arenas (a net that is not re-packed, or a missed step counter, shows only there).

    Arg-max priors: layouts a and b each differ from the fixture at ONE of 312 positions (x3 and x2 alike); a mismatch is accepted only
    at a tie (margin below 1e-4 in the HIP step's own distribution), at most two.

    Clip norms: the last stage's own SR net (layouts a, b) at 3e-3 (measured <= 1.6e-4).  Every other SR net's gradient is dominated at
    N 4 by its STN head, whose gradient reaches it through the TPS sampler (piecewise-linear in the grid, the head starting near the
    identity) and, for the earlier stages, through the later stages' students.  That value is ill-conditioned in fp32: the CPU oracle's
    own result for layout a's first net moves with the reduction order (1520.97 / 1529.38 / 1535.26 at 8 / 1 / 3 threads; fp64 1520.79),
    its fp32 STN-head tensors were 9.5e-2 away from its fp64 ones on the GPU host, and there even the fp64 value was 1606.5 (a host
    difference not traced further).  Those nets are held at 1e-1 (measured up to 7.2e-2 against the fixture; the full-size test below
    pins them against the oracle on the same host at 2e-2, and the Adam-moment check pins each net's own clip coefficient at 1e-6) --
    enough to see a net that got no gradient or another net's."""
    g, lr, hr, *_ = cascade_models(golden_dir, layout)
    ts, srs, stus, *_ = _step(layout, (301, 302, 303))
    assert ts.precision == golden_policy.name
    assert len(srs) == len(g[f"{layout}_gnorm"][0])
    lr, hr = lr.to(DEV), hr.to(DEV)
    l0 = ts.step(lr, hr).item()
    gn = [ts.opt.grad_norm(m).item() for m in srs]
    ref_gn = [float(x) for x in g[f"{layout}_gnorm"][0]]
    pv = torch.stack([ts._static["p"][i].cpu().permute(1, 0, 2) for i in range(S)])          # (stage, T, N, C)
    am = pv.argmax(-1).numpy()
    top2 = pv.topk(2, -1).values
    bad = am != g[f"{layout}_prior_argmax_step0"]
    margins = (top2[..., 0] - top2[..., 1])[torch.from_numpy(bad)].tolist()
    moments = _clipped_moment_norms(ts, srs, gn)
    l1 = ts.step(lr, hr).item()
    torch.cuda.synchronize()
    dl = [abs(l0 - g[f"{layout}_loss"][0]) / g[f"{layout}_loss"][0], abs(l1 - g[f"{layout}_loss"][1]) / g[f"{layout}_loss"][1]]
    dgn = [abs(a - b) / b for a, b in zip(gn, ref_gn)]
    print(f"{layout} [{golden_policy.name}]: loss rel err step0 {dl[0]:.2e} step1 {dl[1]:.2e}; clip norms {gn} vs {ref_gn} "
          f"(rel {['%.1e' % x for x in dgn]}); |m| rel err {['%.1e' % x for x in moments]}; arg-max mismatches at stages "
          f"{np.nonzero(bad)[0].tolist()}, top-2 margins {margins}")
    assert dl[0] < golden_policy.tol(3e-4)
    if len(srs) > 1:
        assert dgn[-1] < 3e-3, dgn
    assert max(dgn) < 1e-1, dgn
    assert max(moments) < 1e-6, moments
    # identical arg-max priors, except at a tie: a position whose top-1 / top-2 margin is below 1e-4 (the fixture holds arg-maxes only)
    assert int(bad.sum()) <= 2 and all(m < 1e-4 for m in margins), (int(bad.sum()), margins)
    # step 1 (measured: x3 <= 1.5e-3, x2 <= 5.5e-3; the single-stage C3 test allows 2e-2 there)
    assert dl[1] < 1e-2, dl


@pytest.mark.parametrize("layout", ["a", "b"])
def test_cascade_topology_bs32_vs_oracle(layout):
    """full size, stu_iter 3, STN on, bs 32 (modelled on test_c5_shape_stu_iter3_sr_share_bs32_vs_oracle): loss, |dPSNR| of the last
    stage, identical arg-max priors at every stage, the three clip norms, the clipped Adam moments, the BatchNorm running statistics of
    every SR net and student after one step (a shared student's moved three times, in stage order), and a second replica bitwise.
    Measured: loss 2.3e-7, dPSNR <= 5.7e-6 dB, clip norms <= 1.4e-3, moments <= 7.4e-8, running statistics <= 3.9e-6.  One arg-max
    position of layout a's last stage differs at an oracle top-1 / top-2 margin of 7.3e-7 (a tie the fp32 oracle breaks by rounding
    after three cascaded stages): mismatches are allowed only at margins below 1e-5."""
    _threads()
    sr_share, tpg_share = LAYOUTS[layout]
    ts, srs, stus, sds, sd_s, sd_t = _step(layout, (21, 22, 23))
    lr, hr = O.synthetic_batch(32, 555)
    loss = ts.step(lr.to(DEV), hr.to(DEV))
    torch.cuda.synchronize()
    ps, pu, pt = [O.as_params(x) for x in sds], [O.as_params(x) for x in sd_s], O.as_params(sd_t, False)
    opt = O.AdamState([q[k] for q in ps + pu for k in O.trainable_keys(q)])
    ref = O.tpgsr_train_step(ps, pu, pt, opt, lr, hr, stu_iter=S, sr_share=sr_share, tpg_share=tpg_share)
    dloss = abs(loss.item() - ref["loss"].item()) / ref["loss"].item()
    dpsnr = abs(_psnr(ts.last_sr, hr) - _psnr(ref["sr"], hr))
    gn = [ts.opt.grad_norm(m).item() for m in srs]
    dgn = [abs(a - float(b)) / float(b) for a, b in zip(gn, ref["grad_norms"])]
    moments = _clipped_moment_norms(ts, srs, gn)
    mism = [argmax_mismatches(ts._static["p"][i].cpu().permute(1, 0, 2), ref["priors"][i]) for i in range(S)]
    bn = []
    for mods, refs in ((srs, ps), (stus, pu)):
        for m, q in zip(mods, refs):
            worst = 0.0
            for k, v in m.state_dict().items():
                if k.endswith("running_mean") or k.endswith("running_var"):
                    r = q[k].detach()
                    worst = max(worst, (v.cpu() - r).abs().max().item() / max(1.0, r.abs().max().item()))
            bn.append(worst)
    print(f"layout {layout} bs32: loss rel err {dloss:.2e}; dPSNR {dpsnr:.2e} dB; clip norms {gn} (rel err {['%.1e' % x for x in dgn]}); "
          f"|m| rel err {['%.1e' % x for x in moments]}; arg-max mismatches per stage {mism}; BN running stats max err "
          f"{['%.1e' % x for x in bn]}")
    assert dloss < 5e-4
    assert dpsnr < 1e-3
    assert all(m == 0 or margin < 1e-5 for m, margin in mism) and sum(m for m, _ in mism) <= 2, mism
    assert max(dgn) < 2e-2, dgn
    assert max(moments) < 1e-6, moments
    assert max(bn) < 2e-5, bn
    ts2, *_ = _step(layout, (21, 22, 23))
    loss2 = ts2.step(lr.to(DEV), hr.to(DEV))
    torch.cuda.synchronize()
    assert loss2.item() == loss.item()
    assert torch.equal(ts2.pool.flat, ts.pool.flat)


def _double(sd, requires_grad=True):
    return O.as_params({k: v.double() if v.is_floating_point() else v for k, v in sd.items()}, requires_grad)


def _unclipped(r, n_sr, groups):
    """the oracle's gradients per group, the SR groups' in-place clip undone (each net its own coefficient)"""
    out, ofs = [], 0
    for j, n in enumerate(groups):
        c = min(1.0, 0.25 / (float(r["grad_norms"][j]) + 1e-6)) if j < n_sr else 1.0
        out.append([g.double() / c for g in r["grads"][ofs:ofs + n]])
        ofs += n
    return out


def _rel(a, b):
    num = sum((x.double() - y).pow(2).sum().item() for x, y in zip(a, b))
    return (num / sum(y.pow(2).sum().item() for y in b)) ** 0.5


@pytest.mark.parametrize("layout", ["a", "b"])
def test_cascade_topology_raw_gradients_vs_fp64(layout):
    """forward + backward only (`_phase_a`, no optimiser), N 4, no STN, stu_iter 3: every gradient against the oracle run in fp64
    (parameters, buffers and inputs cast to double; every oracle piece runs in fp64).
    * the last stage's SR net receives its own image loss's gradient only: its global relative error is pinned at 5e-5 (measured
      9.6e-6 / 1.3e-5, the oracle's own fp32 error against fp64 1.1e-5 / 1.2e-5);
    * every other network -- the earlier stages' SR nets (whose images reach the loss again through the next stage's student and
      prior) and the students (test_cascade_two_stages_vs_oracle) -- carries the ill-conditioned gradient through the text prior: the
      oracle's OWN fp32 result is 2e-3 .. 2e-2 away from fp64 there.  Each is held to twice that plus a small floor; a shared
      student's sum over three stages included (an overwritten instead of accumulated stage shows as O(1))."""
    _threads()
    sr_share, tpg_share = LAYOUTS[layout]
    ts, srs, stus, sds, sd_s, sd_t = _step(layout, (301, 302, 303), stn=False)
    lr, hr = O.synthetic_batch(4, 77)
    ts.pool.bind(torch.device(DEV, 0))
    ts.teacher._engine().bind(torch.device(DEV, 0))
    loss = ts._phase_a(lr.to(DEV), hr.to(DEV))
    torch.cuda.synchronize()
    groups = [len(O.trainable_keys(O.as_params(x))) for x in sds + sd_s]
    refs = {}
    for dt in (torch.float32, torch.float64):
        cast = (lambda sd, rg=True: O.as_params(sd, rg)) if dt == torch.float32 else _double
        ps, pu, pt = [cast(x) for x in sds], [cast(x) for x in sd_s], cast(sd_t, False)
        opt = O.AdamState([q[k] for q in ps + pu for k in O.trainable_keys(q)])
        r = O.tpgsr_train_step(ps, pu, pt, opt, lr.to(dt), hr.to(dt), stu_iter=S, sr_share=sr_share, tpg_share=tpg_share, stn=False)
        refs[dt] = (r["loss"].item(), _unclipped(r, len(sds), groups))
    assert abs(loss.item() - refs[torch.float64][0]) < 3e-4 * refs[torch.float64][0]
    g64, g32 = refs[torch.float64][1], refs[torch.float32][1]
    mine = []
    for m, sd in zip(srs + stus, sds + sd_s):
        P = dict(m.named_parameters())
        mine.append([P[k].grad.detach().cpu() for k in O.trainable_keys(O.as_params(sd))])
    err = [(_rel(mine[j], g64[j]), _rel(g32[j], g64[j])) for j in range(len(groups))]
    print(f"layout {layout}: (HIP, oracle fp32) vs fp64, SR nets {[('%.2e' % a, '%.2e' % b) for a, b in err[:S]]}, students "
          f"{[('%.2e' % a, '%.2e' % b) for a, b in err[S:]]}")
    assert err[S - 1][0] < 5e-5, err[S - 1]
    for a, b in err[:S - 1] + err[S:]:
        assert a <= 2 * b + 2e-3, err


def test_shared_student_three_stream_equals_serial_and_graph_replay(schedule):
    """layout b (three SR nets, one shared student) at bs 32, 2 steps: the default three-stream schedule == the serial one (losses,
    parameters, gradients) bit for bit -- a fresh replica recording its OWN plans in serial mode (recording-time stream decisions) and
    the three-stream plans themselves replayed serially -- and the step captured into a hipGraph and replayed == eager, bitwise"""
    K = schedule
    lr, hr = O.synthetic_batch(32, 555)
    lr, hr = lr.to(DEV), hr.to(DEV)
    ts, srs, stus, sds, sd_s, _ = _step("b", (31, 32, 33))
    la, pa, ga = _run(ts, lr, hr, 2)
    K.set_schedule(serial=True)
    ts2, *_ = _step("b", (31, 32, 33))
    lb, pb, gb = _run(ts2, lr, hr, 2)
    K.set_schedule()
    del ts2
    _reset(ts, sds + sd_s)
    K.set_schedule(serial=True)
    lc, pc, gc = _run(ts, lr, hr, 2)
    K.set_schedule()
    print("default", la, "serial (own plans)", lb, "serial (same plans)", lc)
    assert la == lb == lc
    assert torch.equal(pa, pb) and torch.equal(ga, gb)
    assert torch.equal(pa, pc) and torch.equal(ga, gc)
    ea, *_ = _step("b", (31, 32, 33))
    eb, *_ = _step("b", (31, 32, 33))
    eb.capture(lr, hr, warmup=1)
    le = [ea.step(lr, hr).item() for _ in range(3)]
    lg = [eb.replay().item() for _ in range(2)]
    torch.cuda.synchronize()
    print("eager", le, "replay", lg)
    assert lg[0] == le[1] and lg[1] == le[2]
    assert torch.equal(ea.pool.flat, eb.pool.flat)
