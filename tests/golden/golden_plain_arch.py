"""What the generators of the prior-free backbones share (make_golden_lapsrn.py, make_golden_rrdb.py, make_golden_edsr.py): the float64
SSIM over the reference's window, `to64`, the float32-against-float64 error measures, the bounds the GPU tests apply (`BOUNDS`, held to a
quarter by the reference's own float32 run) and the skeletons of the model, train and evaluator fixtures over a `Recipe` -- one backbone's
constructor, float64 restatement, frozen tensors and batch sizes.  The reference is never imported here: a generator's main() does that
and hands it in as `R`."""
import dataclasses
import math
import os
from typing import Callable

import numpy as np
import torch
import torch.nn.functional as F

from make_golden_next import generic_recipe, grad_summary

# the bounds of tests/plain_arch_common.py for the quantities a fixture holds
BOUNDS = dict(fwd=1e-4, grad=5e-3, head=0.1, loss=3e-4, gnorm=3e-3, loss2=2e-2, dpsnr=1e-5, dssim=1e-7)


def ssim_window(window_size=11, taps=torch.float32):
    """the taps of utils/ssim_psnr.py:18-27 gaussian / create_window as a float32 tensor.  taps=float32 (RRDBNet, EDSR) is how the reference
    builds them: the Gaussian from Python floats into a float32 tensor, normalised and multiplied out IN FLOAT32.  They sum to 1 - 6.9e-8;
    taps=float64 (LapSRN) builds them in float64 and rounds afterwards, they sum to 1 - 6.2e-9, and on the RRDBNet evaluator batches that
    alone moves the mean SSIM by 1.1e-7 (x2) / 2.1e-8 (x4): the generators assert the float32 taps against the reference's own"""
    if taps == torch.float32:
        g = torch.Tensor([math.exp(-(x - window_size // 2) ** 2 / float(2 * 1.5 ** 2)) for x in range(window_size)])
    else:
        g = torch.exp(-(torch.arange(window_size, dtype=torch.float64) - window_size // 2) ** 2 / (2 * 1.5 ** 2))
    g = (g / g.sum()).unsqueeze(1)
    return g.mm(g.t()).float()


def ssim64(img1, img2, window_size=11, taps=torch.float32):
    """utils/ssim_psnr.py SSIM(window_size=11, size_average=True) in the dtype of its inputs over ssim_window(window_size, taps)"""
    a, b = img1[:, :3], img2[:, :3]
    ch = a.shape[1]
    w = ssim_window(window_size, taps).to(a.dtype).expand(ch, 1, window_size, window_size).contiguous()
    pd = window_size // 2
    mu1, mu2 = F.conv2d(a, w, padding=pd, groups=ch), F.conv2d(b, w, padding=pd, groups=ch)
    s11 = F.conv2d(a * a, w, padding=pd, groups=ch) - mu1 * mu1
    s22 = F.conv2d(b * b, w, padding=pd, groups=ch) - mu2 * mu2
    s12 = F.conv2d(a * b, w, padding=pd, groups=ch) - mu1 * mu2
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    return (((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s11 + s22 + c2))).mean()


def to64(sd):
    return {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}


@dataclasses.dataclass(frozen=True)
class Recipe:
    build: Callable                 # (R, scale, nb) -> the reference's module
    forward: Callable               # (p, x, scale, nb) -> the float64 restatement
    channels: int
    n: dict                         # depth -> batch size
    n_store: dict                   # scale -> samples of a 16x64 batch whose SR image is stored
    n_small: int
    small_hw: tuple
    eval_n: int
    eval_nb: int
    eval_seeds: dict
    eval_data_seeds: range
    frozen: tuple = ()              # parameters without gradient, left bit for bit by the optimiser
    fwd_tol: float = 0.25 * BOUNDS["fwd"]      # float32 reference against float64, of max(1, |y| max)
    metric_margin: bool = True      # an evaluator batch has to leave three quarters of the metric bounds to the device


class OverMargin(AssertionError):
    pass


def _rel(a, b):
    return float((a.double() - b.double()).abs().max()) / max(1.0, float(b.double().abs().max()))


def _within(err, tol, what):
    if not err <= tol:
        raise OverMargin(f"{what}: the reference's float32 run is {err:.2e} from float64, more than {tol:.1e}")
    return err


def _quarter(err, bound, what):
    return _within(err, 0.25 * bound, f"{what} (a quarter of the bound {bound:.0e})")


def _grad_errors(net32, p64, frozen=()):
    """the per-parameter rule of check_param_grads (tests/test_tl_cascade_gpu.py), float32 reference against float64; frozen tensors have
    no gradient on either side"""
    n64 = {k: float(v.grad.norm()) for k, v in p64.items() if v.grad is not None}
    gmax = max(n64.values())
    en = eh = 0.0
    worst = None
    for k, q in net32.named_parameters():
        if k in frozen:
            assert q.grad is None and p64[k].grad is None, k
            continue
        g32, g64 = q.grad.double(), p64[k].grad
        e = abs(float(g32.norm()) - n64[k]) / max(n64[k], 1e-3 * gmax)
        if e > en:
            en, worst = e, k
        sc = max(n64[k], 1e-3 * gmax) / np.sqrt(g64.numel())
        eh = max(eh, float((g32.reshape(-1)[:8] - g64.reshape(-1)[:8]).abs().max()) / sc)
    print(f"  worst parameter-gradient norm: {worst} {en:.2e} (|g| {n64[worst]:.3e}, largest {gmax:.3e})")
    return en, eh


def _p64(sd, frozen):
    p = to64(sd)
    for k, v in p.items():
        if k not in frozen:
            v.requires_grad_(True)
    return p


def model_fixture(rc, nb, s, seeds, R, O):
    dseed, wseed, gseed, sseed = seeds
    lr = O.synthetic_batch(rc.n[nb], dseed, scale=s)[0][:, :rc.channels].contiguous()
    lr_s = O.synthetic_batch(rc.n_small, sseed, lr_hw=rc.small_hw, scale=s)[0][:, :rc.channels].contiguous()
    ref = rc.build(R, s, nb)
    sd = generic_recipe(ref.state_dict(), wseed)
    ref.load_state_dict(sd, strict=True)
    assert [k for k, q in ref.named_parameters() if not q.requires_grad] == list(rc.frozen)
    ref.eval()
    with torch.no_grad():
        ys = ref(lr_s)
        _within(_rel(ys, rc.forward(to64(sd), lr_s.double(), s, nb)), rc.fwd_tol, f"nb {nb} x{s} eval 12x40")
    ref.train()
    y = ref(lr)
    gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(gseed))
    (y * gy).sum().backward()
    p64 = _p64(sd, rc.frozen)
    y64 = rc.forward(p64, lr.double(), s, nb)
    e = _within(_rel(y.detach(), y64.detach()), rc.fwd_tol, f"nb {nb} x{s} train")
    (y64 * gy.double()).sum().backward()
    en, eh = _grad_errors(ref, p64, rc.frozen)
    _quarter(en, BOUNDS["grad"], f"nb {nb} x{s} parameter-gradient norms")
    _quarter(eh, BOUNDS["head"], f"nb {nb} x{s} parameter-gradient heads")
    names, norms, heads = grad_summary(ref)
    print(f"nb {nb} x{s}: y {tuple(y.shape)}, {len(names)} parameters, |y| max {float(y.abs().max()):.3f}; float32 against float64: forward "
          f"{e:.2e}, gradient norms {en:.2e}, heads {eh:.2e}")
    pre = f"nb{nb}_"
    return {pre + "y": y.detach().numpy()[:rc.n_store[s]], pre + "y_small": ys.numpy(), pre + "grad_names": names, pre + "grad_norms": norms,
            pre + "grad_heads": heads, pre + "seeds": np.array([dseed, wseed, gseed, sseed])}


def train_fixture(rc, nb, s, seeds, R, O):
    """two steps of the reference loop body (:409-424): nn.L1Loss()(model(lr[:, :3]), hr[:, :3]).mean() * 100, clip 0.25, Adam(lr 1e-3,
    betas (0.5, 0.999)) over model.parameters() -- and the same two steps in float64 over the restatement"""
    dseed, wseed, _, _ = seeds
    C = rc.channels
    lr, hr = O.synthetic_batch(rc.n[nb], dseed, scale=s)
    net = rc.build(R, s, nb)
    sd = generic_recipe(net.state_dict(), wseed)
    net.load_state_dict(sd)
    net.train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3, betas=(0.5, 0.999))
    crit = torch.nn.L1Loss()
    p64 = _p64(sd, rc.frozen)
    train64 = [v for k, v in p64.items() if k not in rc.frozen]
    opt64 = torch.optim.Adam(train64, lr=1e-3, betas=(0.5, 0.999))
    loss_l, gn_l = [], []
    for step in range(2):
        sr = net(lr[:, :C, ...])
        loss = crit(sr, hr[:, :C, ...]).mean() * 100
        opt.zero_grad()
        loss.backward()
        if step == 0:
            gs = grad_summary(net)
            sr0 = sr.detach().numpy()[:rc.n_store[s]]
        gn = torch.nn.utils.clip_grad_norm_(net.parameters(), 0.25)
        opt.step()
        sr64 = rc.forward(p64, lr[:, :C].double(), s, nb)
        loss64 = (sr64 - hr[:, :C].double()).abs().mean() * 100
        opt64.zero_grad()
        loss64.backward()
        gn64 = torch.nn.utils.clip_grad_norm_(train64, 0.25)
        opt64.step()
        _quarter(abs(loss.item() - loss64.item()) / loss64.item(), BOUNDS["loss" if step == 0 else "loss2"], f"nb {nb} x{s} loss, step {step}")
        if step == 0:
            _quarter(abs(float(gn) - float(gn64)) / float(gn64), BOUNDS["gnorm"], f"nb {nb} x{s} clip norm")
            _within(_rel(sr.detach(), sr64.detach()), rc.fwd_tol, f"nb {nb} x{s} sr_step0")
        loss_l.append(loss.item())
        gn_l.append(float(gn))
        print(f"  nb {nb} x{s} step {step}: loss {loss.item():.6f} (float64 {loss64.item():.6f})  clip norm {float(gn):.5f} (float64 {float(gn64):.5f})")
    for k in rc.frozen:                                            # torch.optim.Adam skips parameters without a gradient
        assert torch.equal(net.state_dict()[k], sd[k]), k
    pre = f"nb{nb}_"
    return {pre + "loss": np.array(loss_l), pre + "gnorm": np.array(gn_l), pre + "sr_step0": sr0, pre + "sr_grad_names": gs[0],
            pre + "sr_grad_norms": gs[1], pre + "sr_grad_heads": gs[2], pre + "seeds": np.array([dseed, wseed])}


def eval_fixture(rc, s, R, O):
    """the evaluator batch of a factor: the first data seed at which the recogniser's float32 and float64 arg-max agree at every time step
    for LR, HR and the SR image; the expected strings = the oracle's CRNN forward + greedy decode on the reference SR image"""
    C = rc.channels
    sd_r = O.recipe_state_dict(O.crnn_spec(), rc.eval_seeds["rec"])
    r32, r64 = O.as_params(sd_r, False), O.as_params(to64(sd_r), False)
    ref = rc.build(R, s, rc.eval_nb)
    sd = generic_recipe(ref.state_dict(), rc.eval_seeds[s])
    ref.load_state_dict(sd, strict=True)
    ref.eval()

    def logits(img, p):
        return O.crnn_forward(p, O.parse_crnn_data(img[:, :3]), training=False)

    with torch.no_grad():
        for tried, seed in enumerate(rc.eval_data_seeds, 1):
            lr, hr = O.synthetic_batch(rc.eval_n, seed, scale=s)
            sr = ref(lr[:, :C])
            sr64 = rc.forward(to64(sd), lr[:, :C].double(), s, rc.eval_nb)
            _within(_rel(sr, sr64), rc.fwd_tol, f"evaluator x{s} SR")
            if rc.metric_margin:
                # the metrics of the reference's float32 image against those of the float64 image, both computed in float64: a batch on
                # which the reference's own rounding uses up more than a quarter of the evaluator test's metric bounds is no fixture for them
                hr64 = hr[:, :C].double()
                dp = abs(float(O.calculate_psnr(sr.double(), hr64)) - float(O.calculate_psnr(sr64, hr64)))
                ds = abs(float(ssim64(sr.double(), hr64)) - float(ssim64(sr64, hr64)))
                if dp > 0.25 * BOUNDS["dpsnr"] or ds > 0.25 * BOUNDS["dssim"]:
                    print(f"  evaluator batch x{s} seed {seed}: the float32 reference image moves PSNR by {dp:.2e} dB, SSIM by {ds:.2e}, next seed")
                    continue
            res, ok = {}, True
            for k, img in (("lr", lr), ("hr", hr), ("sr", sr)):
                l32, l64 = logits(img, r32), logits(img.double(), r64)
                if not torch.equal(l32.argmax(-1), l64.argmax(-1)):
                    ok = False
                    break
                res[k] = O.get_string_crnn(l32)
            if not ok:
                print(f"  evaluator batch x{s} seed {seed}: float32 / float64 arg-max differ, next seed")
                continue
            print(f"evaluator batch x{s}: data seed {seed} ({tried} tried)", res)
            return dict(eval_seed=np.array(seed), eval_lr=np.array(res["lr"]), eval_hr=np.array(res["hr"]), eval_sr=np.array(res["sr"]))
    raise RuntimeError("no evaluator batch with agreeing float32 / float64 arg-max among the candidate seeds")


def save_pair(out_dir, stem, s, model, train):
    for f, d in ((f"{stem}_x{s}.npz", model), (f"train_{stem}_x{s}.npz", train)):
        np.savez_compressed(os.path.join(out_dir, f), **d)
        assert os.path.getsize(os.path.join(out_dir, f)) < 700 * 1024, f
