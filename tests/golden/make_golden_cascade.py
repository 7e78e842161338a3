#!/usr/bin/env python
"""BUILD CONTAINER ONLY: fixtures of the multi-stage cascade with the reference's default topology flags (main.py:44-45: `--sr_share` and
`--tpg_share` both off) and with one shared text-prior generator (`--tpg_share`).  Composes the cascade loop body exactly as
interfaces/super_resolution.py:295-424 does, from the genuine reference's modules (oracle/ref_import.py): teacher CRNN on HR, per stage
student CRNN (`tpg_pick`, :307-311) -> softmax -> distill loss -> prior with samples [0, N//4) zeroed -> SR net (`model_list[pick]`,
:354-358 / :90-94) -> image loss; ONE torch.optim.Adam over SR nets + students; clip_grad_norm_(0.25) per SR net in `model_list`
(:421-422).  Hard-asserts oracle.tpgsr_train_step == that composition on every recorded number and writes
tests/golden/train_cascade_topologies.npz (numbers only: the weights come from the recipe seeds, the batch from
oracle.synthetic_batch).

Layouts, stu_iter 3, N 4, STN on, two steps each:
  a  sr_share=False, tpg_share=False   three TSRN_TL, three students (the reference's default)
  b  sr_share=False, tpg_share=True    three TSRN_TL, one student
  c  sr_share=True,  tpg_share=True    one TSRN_TL, one student"""
import io
import os
import sys
import zipfile

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import ref_import, tpgsr_oracle as O  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
N, STU_ITER, STEPS, BATCH_SEED, THREADS = 4, 3, 2, 71, 8
SR_SEED, TEACHER_SEED, STU_SEED = 301, 302, 303          # net k: seed + 10 k (tests/test_crnn_gpu.py:_c3_models)
LAYOUTS = {"a": (False, False), "b": (False, True), "c": (True, True)}
# oracle vs reference, relative: step 0 runs the same arithmetic; step 1 follows Adam's first update, where m / sqrt(v) turns
# rounding-level gradient differences into +-lr steps (make_golden.py, C2 notes)
LOSS_TOL = (1e-5, 2e-5)
GNORM_TOL = (1e-4, 5e-3)
SUM_TOL = (1e-6, 1e-5)


def checksum(state):
    return float(sum(v.double().abs().sum() for v in state.values() if v.is_floating_point()))


def save_npz(path, data):
    """np.savez_compressed with a fixed member timestamp: a re-run on the same host reproduces the file bit for bit"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, v in data.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), compress_type=zipfile.ZIP_DEFLATED)


def close(a, b, tol, what):
    a, b = float(a), float(b)
    err = abs(a - b) / max(1.0, abs(b))
    assert err <= tol, f"{what}: oracle {a} vs reference {b} (rel {err:.2e})"
    return err


def run(R, lr, hr, sr_share, tpg_share, tag):
    n_sr, n_stu = (1 if sr_share else STU_ITER), (1 if tpg_share else STU_ITER)
    sd_sr = [O.recipe_state_dict(O.tsrn_spec(STN=True, mask=True, text_prior=True), SR_SEED + 10 * k, tps_hw=(16, 64)) for k in range(n_sr)]
    sd_s = [O.recipe_state_dict(O.crnn_spec(), STU_SEED + 10 * k) for k in range(n_stu)]
    sd_t = O.recipe_state_dict(O.crnn_spec(), TEACHER_SEED)
    model_list = []
    for sd in sd_sr:
        m = R.tsrn.TSRN_TL(STN=True, mask=True); m.load_state_dict(sd); model_list.append(m.train())
    teacher = R.crnn.CRNN(32, 1, 37, 256); teacher.load_state_dict(sd_t); teacher.eval()
    for q in teacher.parameters():
        q.requires_grad = False
    students = []
    for sd in sd_s:
        s = R.crnn.CRNN(32, 1, 37, 256); s.load_state_dict(sd); students.append(s.train())
    opt = torch.optim.Adam([q for m in model_list + students for q in m.parameters()], lr=1e-3, betas=(0.5, 0.999))
    sem, crit = R.semantic_loss.SemanticLoss(), R.image_loss.ImageLoss(gradient=True, loss_weight=[1, 1e-4])
    ps, pu, pt = [O.as_params(x) for x in sd_sr], [O.as_params(x) for x in sd_s], O.as_params(sd_t, False)
    oopt = O.AdamState([q[k] for q in ps + pu for k in O.trainable_keys(q)])
    rec = {k: [] for k in ("loss", "loss_img", "loss_distill", "gnorm", "checksum_sr", "checksum_stu")}
    worst = {}
    for step in range(STEPS):
        # interfaces/super_resolution.py:295-406
        label_vecs_hr = F.softmax(teacher(O.parse_crnn_data(hr[:, :3])).detach(), -1)
        cascade = lr
        loss_img, loss_distill, priors = 0., 0., []
        for i in range(STU_ITER):
            stu_model = students[0 if tpg_share else i]
            label_vecs = F.softmax(stu_model(O.parse_crnn_data(cascade[:, :3])), -1)
            label_vecs_final = label_vecs.permute(1, 0, 2).unsqueeze(1).permute(0, 3, 1, 2)
            loss_distill = loss_distill + sem(label_vecs, label_vecs_hr) * 100
            drop_vec = torch.ones(N).float()
            drop_vec[:N // 4] = 0.
            label_vecs_final = label_vecs_final * drop_vec.view(-1, 1, 1, 1)
            cascade = model_list[0 if sr_share else i](lr, label_vecs_final)
            loss_img = loss_img + crit(cascade, hr).mean() * 100
            priors.append(label_vecs.detach())
        loss = loss_img + loss_distill
        opt.zero_grad(); loss.backward()
        gn = [float(torch.nn.utils.clip_grad_norm_(m.parameters(), 0.25)) for m in model_list]      # :421-422
        opt.step()
        r = O.tpgsr_train_step(ps, pu, pt, oopt, lr, hr, stu_iter=STU_ITER, sr_share=sr_share, tpg_share=tpg_share)
        what = f"{tag} step{step}"
        for key, ref in (("loss", loss), ("loss_img", loss_img), ("loss_distill", loss_distill)):
            worst[key] = close(r[key], ref, LOSS_TOL[step], f"{what} {key}")
        for k in range(n_sr):
            worst[f"gnorm[{k}]"] = close(r["grad_norms"][k], gn[k], GNORM_TOL[step], f"{what} gnorm[{k}]")
        cs_sr, cs_stu = [checksum(m.state_dict()) for m in model_list], [checksum(m.state_dict()) for m in students]
        for k in range(n_sr):
            worst[f"checksum SR[{k}]"] = close(checksum(ps[k]), cs_sr[k], SUM_TOL[step], f"{what} checksum SR[{k}]")
        for k in range(n_stu):
            worst[f"checksum student[{k}]"] = close(checksum(pu[k]), cs_stu[k], SUM_TOL[step], f"{what} checksum student[{k}]")
        print(f"  {tag} step {step} oracle vs reference, worst relative: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
        worst.clear()
        if step == 0:
            argmax = np.stack([p.argmax(-1).numpy() for p in priors])              # (stage, T, N)
            assert (np.stack([p.argmax(-1).numpy() for p in r["priors"]]) == argmax).all(), f"{what} arg-max priors"
        rec["loss"].append(loss.item()); rec["loss_img"].append(float(loss_img)); rec["loss_distill"].append(float(loss_distill))
        rec["gnorm"].append(gn); rec["checksum_sr"].append(cs_sr); rec["checksum_stu"].append(cs_stu)
        print(f"  {tag} step {step}: loss {loss.item():.6f} (img {float(loss_img):.5f} distill {float(loss_distill):.5f}) "
              f"gnorms {[round(g, 4) for g in gn]}")
    out = {f"{tag}_{k}": np.array(v) for k, v in rec.items()}
    out[f"{tag}_prior_argmax_step0"] = argmax.astype(np.int8)
    return out


def main():
    R = ref_import.load()
    torch.manual_seed(0)
    torch.set_num_threads(THREADS)          # CPU reduction order, hence every bit of the fixture, depends on the thread count
    lr, hr = O.synthetic_batch(N, BATCH_SEED)
    data = dict(n=N, stu_iter=STU_ITER, batch_seed=BATCH_SEED, seeds=np.array([SR_SEED, TEACHER_SEED, STU_SEED]),
                layouts=np.array(list(LAYOUTS)), sr_share=np.array([v[0] for v in LAYOUTS.values()]),
                tpg_share=np.array([v[1] for v in LAYOUTS.values()]),
                checksum_lr=checksum({"lr": lr}), checksum_hr=checksum({"hr": hr}))
    for tag, (sr_share, tpg_share) in LAYOUTS.items():
        data.update(run(R, lr, hr, sr_share, tpg_share, tag))
    path = os.path.join(OUT, "train_cascade_topologies.npz")
    save_npz(path, data)
    print(f"{os.path.basename(path)} written ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
