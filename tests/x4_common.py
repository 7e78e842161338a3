"""scale_factor = 4 (two up-sampling stages) -- what the x4 tests share.

The frozen oracle restates the x4 NETWORK (`tpgsr_oracle.tsrn_forward(..., scale_factor=4)`), but its step-level functions
(`tsrn_train_step`, `tpgsr_train_step`, `tpgsr_eval_step`) do not pass a scale.  They are restated here, composed from the oracle's own
parts -- same operations in the same order, plus `scale_factor=` -- and tests/test_x4_cpu.py pins them bitwise (float64, scale_factor = 2)
against the oracle's before anything leans on them.  Everything runs in the dtype of the parameters handed in: float64 for the GPU
tests' reference, float32 where a number is compared with the reference's own (tests/golden/make_golden_x4.py)."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import tpgsr_oracle as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
X4_KW = dict(scale_factor=4, width=256, height=64, STN=True, mask=True)      # the natural x4 configuration: LR 16x64 -> SR 64x256


def params(sd, requires_grad=True, dtype=torch.float64):
    """O.as_params in `dtype`"""
    return O.as_params({k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}, requires_grad)


def prior_from_seed(n, seed):
    return F.softmax(torch.randn(n, 37, 1, 26, generator=torch.Generator().manual_seed(seed)) * 2, 1)


# ---- restated steps ---------------------------------------------------------------------------------------------------------------
def tsrn_train_step(p, opt, lr_img, hr_img, *, scale_factor=2, stn=True, srb_nums=5, gradient=True, explicit_rnn=False,
                    grid_align_corners=False):
    """O.tsrn_train_step (config C2) with the network's scale"""
    sr = O.tsrn_forward(p, lr_img, training=True, stn=stn, srb_nums=srb_nums, explicit_rnn=explicit_rnn,
                        grid_align_corners=grid_align_corners, scale_factor=scale_factor)
    loss = O.image_loss(sr, hr_img, gradient).mean() * 100
    keys = O.trainable_keys(p)
    grads = list(torch.autograd.grad(loss, [p[k] for k in keys]))
    gnorm = O.clip_grad_norm_(grads, 0.25)
    opt.step(grads)
    return {"loss": loss.detach(), "grad_norm": gnorm, "sr": sr.detach(), "grads": dict(zip(keys, grads))}


def tpgsr_train_step(sr_params, stu_params, teacher, opt, lr_img, hr_img, *, scale_factor=2, stu_iter=1, sr_share=True, tpg_share=False,
                     stn=True, srb_nums=5, gradient=True, explicit_rnn=False, grid_align_corners=False):
    """O.tpgsr_train_step (configs C3-C5, `--use_distill`, CRNN text-prior generator) with the SR networks' scale"""
    tpg_forward = lambda q_, g_, training: O.crnn_forward(q_, g_, training=training, explicit_rnn=explicit_rnn)
    with torch.no_grad():
        t_logits = tpg_forward(teacher, O.parse_crnn_data(hr_img[:, :3]), training=False)
        q = F.softmax(t_logits, -1)
    cascade = lr_img
    loss_img = 0.0
    loss_distill = 0.0
    priors, srs = [], []
    for i in range(stu_iter):
        stu = stu_params[0 if tpg_share else i]
        logits = tpg_forward(stu, O.parse_crnn_data(cascade[:, :3]), training=True)
        pv = F.softmax(logits, -1)                                   # (26, N, 37)
        prior = pv.permute(1, 0, 2).unsqueeze(1).permute(0, 3, 1, 2)  # (N, 37, 1, 26)
        loss_distill = loss_distill + O.semantic_loss(pv, q) * 100
        drop = torch.ones(lr_img.shape[0])
        drop[: lr_img.shape[0] // 4] = 0.0
        prior = prior * drop.view(-1, 1, 1, 1)
        priors.append(pv.detach())
        srp = sr_params[0 if sr_share else i]
        cascade = O.tsrn_forward(srp, lr_img, prior, training=True, stn=stn, srb_nums=srb_nums, text_prior=True,
                                 explicit_rnn=explicit_rnn, grid_align_corners=grid_align_corners, scale_factor=scale_factor)
        srs.append(cascade.detach())
        loss_img = loss_img + O.image_loss(cascade, hr_img, gradient).mean() * 100
    loss = loss_img + loss_distill
    groups = [[(m, k) for k in O.trainable_keys(m)] for m in sr_params] + \
             [[(m, k) for k in O.trainable_keys(m)] for m in stu_params]
    flat = [m[k] for grp in groups for (m, k) in grp]
    grads = list(torch.autograd.grad(loss, flat, allow_unused=True))
    grads = [g if g is not None else torch.zeros_like(t) for g, t in zip(grads, flat)]
    ofs = 0
    gnorms = []
    for gi, grp in enumerate(groups):
        if gi < len(sr_params):
            gnorms.append(O.clip_grad_norm_(grads[ofs:ofs + len(grp)], 0.25))
        ofs += len(grp)
    opt.step(grads)
    return {"loss": loss.detach(), "loss_img": torch.as_tensor(loss_img).detach(),
            "loss_distill": torch.as_tensor(loss_distill).detach(), "grad_norms": gnorms,
            "sr": cascade.detach(), "srs": srs, "priors": priors, "grads": grads}


@torch.no_grad()
def tpgsr_eval_step(sr_params, tpg_params, recognizer, lr_img, hr_img, *, scale_factor=2, stu_iter=1, sr_share=True, tpg_share=False,
                    srb_nums=5):
    """O.tpgsr_eval_step with the SR networks' scale"""
    cascade = lr_img
    srs, priors = [], []
    for i in range(stu_iter):
        tpg = tpg_params[0 if tpg_share else i]
        pv = F.softmax(O.crnn_forward(tpg, O.parse_crnn_data(cascade[:, :3]), training=False), -1)
        prior = pv.permute(1, 0, 2).unsqueeze(1).permute(0, 3, 1, 2)
        cascade = O.tsrn_forward(sr_params[0 if sr_share else i], lr_img, prior, training=False, stn=True, srb_nums=srb_nums,
                                 text_prior=True, scale_factor=scale_factor)
        srs.append(cascade)
        priors.append(pv)
    rec = lambda img: O.get_string_crnn(O.crnn_forward(recognizer, O.parse_crnn_data(img[:, :3]), training=False))
    return {"sr": srs, "priors": priors, "psnr": O.calculate_psnr(cascade, hr_img), "ssim": O.ssim(cascade.float(), hr_img.float()),      # (O.ssim's window is float32)
            "pred_sr": rec(cascade), "pred_lr": rec(lr_img), "pred_hr": rec(hr_img)}


def argmax_mismatches(p, p_ref):
    """(number of positions whose arg-max class differs, the reference's top-1 - top-2 probability margin at the worst of them): a mismatch
    at a margin far above rounding noise is a real disagreement, one at 1e-7 a tie the reference itself breaks by rounding"""
    bad = p.argmax(-1) != p_ref.argmax(-1)
    if not bool(bad.any()):
        return 0, 0.0
    top2 = p_ref.topk(2, -1).values
    return int(bad.sum()), float((top2[..., 0] - top2[..., 1])[bad].max())


def adam_for(*param_dicts):
    return O.AdamState([q[k] for q in param_dicts for k in O.trainable_keys(q)])


# ---- fixtures (tests/golden/make_golden_x4.py: seeds, not tensors) ------------------------------------------------------------------
def image_sums(y):
    """per-image sum and sum of squares of a batch (float64): the whole image in two numbers per sample"""
    y = torch.as_tensor(y).double()
    return torch.stack([y.sum((1, 2, 3)), (y * y).sum((1, 2, 3))], 1).numpy()


def model_fixture():
    """model_tsrn_tl_x4.npz and the weights / inputs its seeds stand for"""
    g = np.load(os.path.join(GOLD, "model_tsrn_tl_x4.npz"), allow_pickle=False)
    spec = O.tsrn_spec(text_prior=True, srb_nums=5, **X4_KW)
    sd = O.recipe_state_dict(spec, int(g["weight_seed"]), tps_hw=(16, 64))
    lr, hr = O.synthetic_batch(2, int(g["data_seed"]), scale=4)
    return g, sd, lr, hr, prior_from_seed(2, int(g["prior_seed"]))


def c3_fixture():
    """train_c3_x4.npz and the three networks' weights / the batch its seeds stand for"""
    g = np.load(os.path.join(GOLD, "train_c3_x4.npz"), allow_pickle=False)
    sd_sr = O.recipe_state_dict(O.tsrn_spec(text_prior=True, srb_nums=5, **X4_KW), int(g["sr_seed"]), tps_hw=(16, 64))
    sd_t = O.recipe_state_dict(O.crnn_spec(), int(g["teacher_seed"]))
    sd_s = O.recipe_state_dict(O.crnn_spec(), int(g["student_seed"]))
    lr, hr = O.synthetic_batch(4, int(g["data_seed"]), scale=4)
    return g, sd_sr, sd_t, sd_s, lr, hr


def layout():
    return json.load(open(os.path.join(GOLD, "state_dict_layout_x4.json")))["tsrn_tl_x4"]
