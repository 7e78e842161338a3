#!/usr/bin/env python
"""Reference-pinned fixture for hidden_units = 64 (the reference CLI's `--hd_u 64`): the genuine reference's
TSRN_TL(hidden_units=64, STN=True, mask=True) on recipe weights + seeded inputs, with the CPU oracle pinned against it on the way
(hard asserts, the tolerances of make_golden.py).  Build container only (oracle.ref_import).

srb_nums stays at the reference's default 5: its TSRN_TL.forward hands the text strip to blocks 2..6 by NUMBER (model/tsrn.py:201-209),
so with fewer residual blocks it calls the plain convolution block with two arguments and raises -- the reference runs no other depth.

Run:  python tests/golden/make_golden_hd64.py     (writes model_tsrn_tl_hd64.npz, state_dict_layout_hd64.json)

Data only: seeds, expected outputs, gradient summaries, BatchNorm buffers.  Weights and inputs are NOT stored; both sides regenerate
them from the seeds (recipe_state_dict / synthetic_batch / the prior's generator seed)."""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
from oracle import ref_import  # noqa: E402
from oracle import tpgsr_oracle as O  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
WEIGHT_SEED, DATA_SEED, PRIOR_SEED = 164, 64, 65
torch.manual_seed(0)
torch.set_num_threads(8)


def close(a, b, tol, what=""):
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    err = (a.double() - b.double()).abs().max().item()
    scale = max(1.0, b.double().abs().max().item())
    assert err <= tol * scale, f"{what}: max err {err:.3e} (scale {scale:.3g})"
    return err


def prior_from_seed(n, seed):
    return F.softmax(torch.randn(n, 37, 1, 26, generator=torch.Generator().manual_seed(seed)) * 2, 1)


def main():
    R = ref_import.load()
    kw = dict(hidden_units=64, srb_nums=5, STN=True, mask=True)
    ref = R.tsrn.TSRN_TL(**kw)
    spec = O.tsrn_spec(text_prior=True, **kw)
    layout = [(k, list(v.shape)) for k, v in ref.state_dict().items()]
    assert layout == [(k, list(s)) for k, s, _ in spec], "state_dict layout differs"
    with open(os.path.join(OUT, "state_dict_layout_hd64.json"), "w") as f:
        json.dump({"tsrn_tl_hd64": layout}, f)

    sd = O.recipe_state_dict(spec, WEIGHT_SEED, tps_hw=(16, 64))
    lr, hr = O.synthetic_batch(2, DATA_SEED)
    prior = prior_from_seed(2, PRIOR_SEED)
    loss_fn = lambda y: O.image_loss(y, hr, True, (1, 1e-4)).mean() * 100
    fwd = lambda p, tr, ex: O.tsrn_forward(p, lr, prior, training=tr, stn=True, srb_nums=5, text_prior=True, explicit_rnn=ex)
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
        print(f"  explicit={explicit}: worst rel grad err {worst:.2e}")
    names = list(rg.keys())
    running = {k: v.numpy().copy() for k, v in ref.state_dict().items() if "running_" in k}
    for k, v in running.items():
        close(p[k], v, 1e-5, k)
    ref.load_state_dict(sd, strict=True)
    ref.eval()
    with torch.no_grad():
        y_eval = ref(lr, prior)
        close(fwd(O.as_params(sd, False), False, False), y_eval, 5e-5, "eval fwd")
    np.savez_compressed(
        os.path.join(OUT, "model_tsrn_tl_hd64.npz"), weight_seed=WEIGHT_SEED, data_seed=DATA_SEED, prior_seed=PRIOR_SEED,
        sr_eval=y_eval.numpy(), sr_train=y_ref.detach().numpy(), loss=loss_ref.item(), grad_names=json.dumps(names),
        grad_norms=np.array([float(rg[k].double().norm()) for k in names]), running_names=json.dumps(list(running.keys())),
        running_cat=np.concatenate([v.reshape(-1) for v in running.values()]))
    print("written:", os.path.getsize(os.path.join(OUT, "model_tsrn_tl_hd64.npz")), "bytes")


if __name__ == "__main__":
    main()
