#!/usr/bin/env python
"""Reference-pinned fixtures for scale_factor = 4 (the reference's `down_sample_scale: 4`): the genuine reference's
TSRN_TL(scale_factor=4, width=256, height=64, STN=True, mask=True) on recipe weights + seeded inputs, and a two-step C3-shaped training
trajectory composed from the reference's own modules as make_golden.py does for train_c3.npz.  The CPU oracle (network) and the
restated x4 steps of tests/x4_common.py are pinned against the reference on the way (hard asserts, the tolerances of make_golden.py).
Build container only (oracle.ref_import).

Run:  python tests/golden/make_golden_x4.py     (writes model_tsrn_tl_x4.npz, train_c3_x4.npz, state_dict_layout_x4.json)

Data only: seeds, losses, gradient norms, BatchNorm buffers, the outputs on the [::4, ::4] lattice and per-image sums of the full outputs.
Weights and inputs are NOT stored; both sides regenerate them from the seeds (recipe_state_dict / synthetic_batch / the prior's seed)."""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref_import  # noqa: E402
from oracle import tpgsr_oracle as O  # noqa: E402
import x4_common as X  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
WEIGHT_SEED, DATA_SEED, PRIOR_SEED = 404, 44, 45
SR_SEED, TEACHER_SEED, STUDENT_SEED, C3_DATA_SEED = 341, 342, 343, 64
torch.manual_seed(0)
torch.set_num_threads(8)
F32 = torch.float32


def close(a, b, tol, what=""):
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    err = (a.double() - b.double()).abs().max().item()
    scale = max(1.0, b.double().abs().max().item())
    assert err <= tol * scale, f"{what}: max err {err:.3e} (scale {scale:.3g})"
    return err


def lattice(y):
    return y.detach()[:, :, ::4, ::4].contiguous().numpy()


def model_case(R):
    ref = R.tsrn.TSRN_TL(**X.X4_KW)
    spec = O.tsrn_spec(text_prior=True, srb_nums=5, **X.X4_KW)
    layout = [(k, list(v.shape)) for k, v in ref.state_dict().items()]
    assert layout == [(k, list(s)) for k, s, _ in spec], "state_dict layout differs"
    with open(os.path.join(OUT, "state_dict_layout_x4.json"), "w") as f:
        json.dump({"tsrn_tl_x4": layout}, f)
    sd = O.recipe_state_dict(spec, WEIGHT_SEED, tps_hw=(16, 64))
    lr, hr = O.synthetic_batch(2, DATA_SEED, scale=4)
    assert tuple(lr.shape) == (2, 4, 16, 64) and tuple(hr.shape) == (2, 4, 64, 256)
    prior = X.prior_from_seed(2, PRIOR_SEED)
    loss_fn = lambda y: O.image_loss(y, hr, True, (1, 1e-4)).mean() * 100
    fwd = lambda p, tr, ex: O.tsrn_forward(p, lr, prior, training=tr, stn=True, srb_nums=5, text_prior=True, explicit_rnn=ex, scale_factor=4)
    for explicit in (True, False):
        ref.load_state_dict(sd, strict=True)
        ref.train()
        ref.zero_grad()
        y_ref = ref(lr, prior)
        loss_ref = loss_fn(y_ref)
        loss_ref.backward()
        p = O.as_params(sd)
        y_or = fwd(p, True, explicit)
        loss_or = loss_fn(y_or)
        loss_or.backward()
        close(y_or, y_ref, 5e-5, f"train fwd (explicit={explicit})")
        close(loss_or, loss_ref, 1e-5, "loss")
        rg = {k: q.grad.detach().clone() for k, q in ref.named_parameters() if q.grad is not None}
        gmax = max(v.double().norm().item() for v in rg.values())
        worst = max((p[k].grad.double() - rg[k].double()).norm().item() / max(rg[k].double().norm().item(), 1e-3 * gmax) for k in rg)
        assert worst < 2e-3, f"worst rel grad err {worst}"
        print(f"  x4 model explicit={explicit}: worst rel grad err {worst:.2e}")
    assert tuple(y_ref.shape) == (2, 4, 64, 256)
    names = list(rg.keys())
    running = {k: v.numpy().copy() for k, v in ref.state_dict().items() if "running_" in k}
    for k, v in running.items():
        close(p[k], v, 1e-5, k)
    ref.load_state_dict(sd, strict=True)
    ref.eval()
    with torch.no_grad():
        y_eval = ref(lr, prior)
        close(fwd(O.as_params(sd, False), False, False), y_eval, 5e-5, "eval fwd")
    path = os.path.join(OUT, "model_tsrn_tl_x4.npz")
    np.savez_compressed(
        path, weight_seed=WEIGHT_SEED, data_seed=DATA_SEED, prior_seed=PRIOR_SEED, loss=loss_ref.item(),
        sr_train_lattice=lattice(y_ref), sr_eval_lattice=lattice(y_eval), sr_train_sums=X.image_sums(y_ref.detach()),
        sr_eval_sums=X.image_sums(y_eval), grad_names=json.dumps(names),
        grad_norms=np.array([float(rg[k].double().norm()) for k in names]), running_names=json.dumps(list(running.keys())),
        running_cat=np.concatenate([v.reshape(-1) for v in running.values()]), layout=json.dumps(layout))
    print("written:", path, os.path.getsize(path), "bytes")


def c3_case(R):
    """C3 at x4: TSRN_TL x4 + teacher CRNN + student CRNN, N = 4, two steps (composition of interfaces/super_resolution.py:295-424)"""
    lr, hr = O.synthetic_batch(4, C3_DATA_SEED, scale=4)
    crit = R.image_loss.ImageLoss(gradient=True, loss_weight=[1, 1e-4])
    sd_sr = O.recipe_state_dict(O.tsrn_spec(text_prior=True, srb_nums=5, **X.X4_KW), SR_SEED, tps_hw=(16, 64))
    sd_t = O.recipe_state_dict(O.crnn_spec(), TEACHER_SEED)
    sd_s = O.recipe_state_dict(O.crnn_spec(), STUDENT_SEED)
    net = R.tsrn.TSRN_TL(**X.X4_KW); net.load_state_dict(sd_sr); net.train()
    teacher = R.crnn.CRNN(32, 1, 37, 256); teacher.load_state_dict(sd_t); teacher.eval()
    for q in teacher.parameters():
        q.requires_grad = False
    stu = R.crnn.CRNN(32, 1, 37, 256); stu.load_state_dict(sd_s); stu.train()
    opt = torch.optim.Adam(list(net.parameters()) + list(stu.parameters()), lr=1e-3, betas=(0.5, 0.999))
    sem = R.semantic_loss.SemanticLoss()
    ps, pt, pu = X.params(sd_sr, dtype=F32), X.params(sd_t, False, dtype=F32), X.params(sd_s, dtype=F32)
    oopt = X.adam_for(ps, pu)
    traj = {"loss": [], "loss_img": [], "loss_distill": [], "gnorm": []}
    for step in range(2):
        hr_prior = F.softmax(teacher(O.parse_crnn_data(hr[:, :3])).detach(), -1)
        logits = stu(O.parse_crnn_data(lr[:, :3]))
        pv = F.softmax(logits, -1)
        pf = pv.permute(1, 0, 2).unsqueeze(1).permute(0, 3, 1, 2)
        l_d = sem(pv, hr_prior) * 100
        drop = torch.ones(4); drop[:1] = 0
        pf = pf * drop.view(-1, 1, 1, 1)
        sr = net(lr, pf)
        assert tuple(sr.shape) == (4, 4, 64, 256)
        l_i = crit(sr, hr).mean() * 100
        loss = l_i + l_d
        opt.zero_grad(); loss.backward()
        gn = torch.nn.utils.clip_grad_norm_(net.parameters(), 0.25)
        opt.step()
        r = X.tpgsr_train_step([ps], [pu], pt, oopt, lr, hr, scale_factor=4, stu_iter=1)
        ltol = (1e-4, 5e-4)[step]
        close(r["loss"], loss, ltol, f"C3 x4 step{step} loss"); close(r["grad_norms"][0], gn, 10 * ltol, f"C3 x4 step{step} gnorm")
        if step == 0:
            prior_argmax = pv.detach().argmax(-1).numpy()
            assert (r["priors"][0].argmax(-1).numpy() == prior_argmax).all()
            sr0 = lattice(sr)
            close(r["sr"], sr.detach(), 5e-3, "C3 x4 step0 sr")
        traj["loss"].append(loss.item()); traj["loss_img"].append(l_i.item()); traj["loss_distill"].append(l_d.item())
        traj["gnorm"].append(float(gn))
        print(f"  C3 x4 step {step}: loss {loss.item():.6f} (img {l_i.item():.5f} distill {l_d.item():.5f}) gnorm {float(gn):.5f}")
    path = os.path.join(OUT, "train_c3_x4.npz")
    np.savez_compressed(path, sr_seed=SR_SEED, teacher_seed=TEACHER_SEED, student_seed=STUDENT_SEED, data_seed=C3_DATA_SEED,
                        loss=np.array(traj["loss"]), loss_img=np.array(traj["loss_img"]), loss_distill=np.array(traj["loss_distill"]),
                        gnorm=np.array(traj["gnorm"]), prior_argmax_step0=prior_argmax, sr_step0_lattice=sr0)
    print("written:", path, os.path.getsize(path), "bytes")


def main():
    R = ref_import.load()
    model_case(R)
    c3_case(R)


if __name__ == "__main__":
    main()
