"""The kernels that turn the network's output into the numbers training is judged by -- image loss, semantic loss / text prior, CTC loss,
gradient clipping and Adam (csrc/loss_optim.hip, csrc/crnn.hip) -- against stock PyTorch on the CPU in float64, over the shapes, tails and
edges their single fixture tests leave out.

Method and error rule: tests/kernel_table.py (the `arith` rule of tests/test_functional_ops_gpu.py; for scalars e_ref32 is the maximum over 8
seeds; on top, the limits the fixture tests of the same kernels assert: image loss 1e-6 relative and its gradient 1e-5
(test_kernels_gpu.py::test_image_loss_kernels), SemanticLoss 2e-6 / 1e-5 (test_crnn_gpu.py::test_semantic_loss_module_on_probabilities),
CTC nll 2e-6 and gradient 4e-5 (test_ctc_loss_gpu.py), clip norm 1e-4 and Adam parameters 2e-6 absolute per step
(test_kernels_gpu.py::test_clip_and_adam)).

References:
  image loss     w0 * mse(out, tgt) + w1 * l1(gradmag(out[:, :3]), gradmag(tgt[:, :3])), gradmag by F.pad and slicing as the comment above
                 image_loss_fwd_kernel states it (oracle/tpgsr_oracle.py: image_loss); d out by autograd with a random upstream d loss.
  softmax_prior  softmax; w * (mean |q - p| + mean (q + 1e-20)(log(q + 1e-20) - log(p + 1e-20))); the (N, C, 1, T) prior with the first drop_n
                 samples zeroed; d logits by autograd of loss + <prior, dprior> + <p, dp_in>.
  ctc_loss       F.ctc_loss(log_softmax(x), ..., blank, reduction='none'), gradient of sum(scale * weight * nll), both logit layouts.
  optimiser      torch.nn.utils.clip_grad_norm_ + torch.optim.Adam(betas=(0.5, 0.999)) on a float64 copy, 20+ steps, compared after EVERY step.

Discontinuities: the differentiated cases keep |gradmag(out) - gradmag(tgt)| and |q - p| at least 1e-3 from zero (asserted on the CPU by
test_case_table_is_well_posed); the exact-zero behaviour (sign 0 => no L1 gradient term) is tested separately and exactly.

Infeasible CTC targets (T < L + adjacent repeats): the kernel returns nll = +inf like ATen, and KEEPS A FINITE GRADIENT scale * weight *
softmax(x) (no state is reachable, the occupancy term is 0) where ATen with zero_infinity=False returns NaN for the whole sample.  The
collate cuts labels to 15 and T is 26, so 12 adjacent repeats are needed for this to occur; a NaN would reach every parameter of the
step through the shared backward, the finite value stays inside the sample.  test_ctc_infeasible_target pins both, and that the other
samples of the batch are bit-identical to the batch without the infeasible one.

Observed on an MI355X: worst e_gpu / bound per family (test_zz_report_worst_ratios prints it; 0.25 = as accurate as float32 PyTorch on
the CPU):
  image_loss 0.33, gradient_prior_loss 0.31, softmax_prior 0.22, semantic_loss 0.20, optimiser 0.43, fused_adam 0.42,
  ctc_loss 0.87 (the L = 31 cases: 3.5e-5 on the gradient, the same as float32 ATen's 3.5e-5, against the fixture test's cap of 4e-5).
No family needs more than 4x, with one stated exception: Adam's second moment v carries (1.f - beta2) formed in float32, 1.3e-5 relative
(V_BETA2_TERM below has the derivation; p stays inside its own bound).  Two findings were fixed or pinned with this file: gradmag() in
csrc/loss_optim.hip was contracted differently for `out` and `tgt`, so out == tgt gave sign +-1 instead of 0 (fixed in image_loss_bwd_kernel:
equal central differences decide the tie; every other input keeps its bits); ATen's
CPU CTC backward is not the derivative of its own nll when the LAST label carries the blank's index (test_ctc_last_label_with_the_blanks_index
checks the kernel against central differences instead).
"""
import math

import pytest
import torch
import torch.nn.functional as F

from kernel_table import DEV, F64, FLOOR, MARGIN, KCase, _gen, check_case, check_well_posed, err

FAMILY_KERNELS = {
    "image_loss": {"image_loss_fwd", "image_loss_finalize", "image_loss_bwd"},
    "gradient_prior_loss": {"image_loss_fwd", "image_loss_finalize", "image_loss_bwd"},
    "softmax_prior": {"softmax_prior_fwd", "softmax_prior_bwd", "semantic_loss_finalize"},
    "semantic_loss": {"semantic_loss_fwd", "semantic_loss_bwd", "semantic_loss_finalize"},
    "ctc_loss": {"ctc_loss"},
    "optimiser": {"sumsq_partial", "clip_coef", "clip_coef_steps", "adam_step", "scale_", "step_inc"},
    "fused_adam": {"sumsq_partial", "clip_coef", "clip_coef_steps", "adam_step"},
}
NAMED_IN_THE_ISSUE = {"image_loss_fwd", "image_loss_finalize", "image_loss_bwd", "sumsq_partial", "clip_coef", "clip_coef_steps", "adam_step", "scale_",
                      "step_inc", "softmax_prior_fwd", "softmax_prior_bwd", "semantic_loss_fwd", "semantic_loss_bwd", "semantic_loss_finalize", "ctc_loss"}


def K():
    from tpgsr_amd import kernels
    return kernels


# ---- image loss -------------------------------------------------------------------------------------------------------------
def _gradmag(x):
    from oracle import tpgsr_oracle as O
    return O.gradient_map(x)


def _gm_gap(d64):
    Cc = min(d64["out"].shape[1], 3)
    return (_gradmag(d64["out"][:, :Cc]) - _gradmag(d64["tgt"][:, :Cc])).abs().min().item()


def _il_make(shape, seed):
    """tgt uniform, out = tgt + noise; pixels whose two gradient magnitudes are closer than 2e-3 get a neighbour of `out` moved until none is
    left (the L1 term's sign is then well defined in float32 as well)"""
    g = _gen("image_loss", shape, seed)
    N, C, H, W = shape
    tgt = torch.rand(*shape, generator=g)
    out = tgt + 0.3 * torch.randn(*shape, generator=g)
    dl = torch.rand(1, generator=g) + 0.5
    Cc = min(C, 3)
    for _ in range(500):
        diff = _gradmag(out[:, :Cc].double()) - _gradmag(tgt[:, :Cc].double())
        bad = (diff.abs() < 2 * MARGIN).nonzero()
        if not len(bad):
            break
        n, c, h, w = bad.T
        if W > 1:
            h2, w2 = h, torch.where(w + 1 < W, w + 1, w - 1)
        else:
            h2, w2 = torch.where(h + 1 < H, h + 1, h - 1), w
        delta = (torch.rand(len(bad), generator=g) * 0.1 + 0.05) * (torch.randint(0, 2, (len(bad),), generator=g) * 2 - 1)
        out.index_put_((n, c, h2, w2), delta, accumulate=True)
    else:
        raise AssertionError(f"image loss inputs {shape}: no margin after 500 repairs")
    return {"out": out, "tgt": tgt, "dl": dl}


def _il_ref(d, gradient, w0, w1):
    from oracle import tpgsr_oracle as O
    out = d["out"].clone().requires_grad_(True)
    loss = O.image_loss(out, d["tgt"], gradient, (w0, w1))
    (loss * d["dl"][0]).backward()
    return {"loss": loss.detach().reshape(()), "dout": out.grad}


def _il_gpu_module(d, gradient, w0, w1, prior_loss):
    from tpgsr_amd.loss.image_loss import GradientPriorLoss, ImageLoss
    out = d["out"].clone().requires_grad_(True)
    crit = GradientPriorLoss() if prior_loss else ImageLoss(gradient=gradient, loss_weight=[w0, w1])
    loss = crit(out, d["tgt"])
    (loss * d["dl"][0]).backward()
    return {"loss": loss.detach().reshape(()), "dout": out.grad}


def _il_gpu_raw(d, gradient, w0, w1, nblk):
    k = K()
    out, tgt = d["out"], d["tgt"]
    N, C, H, W = out.shape
    part = torch.full((nblk, 2), float("nan"), device=DEV)
    loss = torch.full((1,), float("nan"), device=DEV)
    dout = torch.full_like(out, float("nan"))
    k.image_loss_fwd(out, tgt, N, C, H, W, gradient, part, nblk)
    k.image_loss_finalize(part, nblk, out.numel(), N * min(C, 3) * H * W if gradient else 0, w0, w1, loss)
    k.image_loss_bwd(out, tgt, d["dl"], N, C, H, W, gradient, w0, w1, dout)
    return {"loss": loss.reshape(()), "dout": dout}


IMAGE_SHAPES = [(2, 1, 5, 7), (1, 2, 4, 6), (2, 3, 6, 9), (2, 4, 16, 64), (1, 4, 1, 13), (3, 3, 9, 1), (1, 4, 2, 2), (1, 1, 1, 2), (4, 4, 32, 128)]
IL_CAPS = {"loss": 1e-6, "dout": 1e-5}


def _image_cases():
    out = []
    for shape in IMAGE_SHAPES:
        sh = "x".join(map(str, shape))
        make = lambda seed, shape=shape: _il_make(shape, seed)
        margin = lambda d64: _margin(_gm_gap(d64), "|gradmag(out) - gradmag(tgt)|")
        for w0, w1 in [(20.0, 1e-4), (1.0, 0.5)]:
            ws = f"w{w0:g}+{w1:g}"
            out.append(KCase("image_loss", f"{sh}-module-{ws}", make, lambda d, w0=w0, w1=w1: _il_ref(d, True, w0, w1),
                             lambda d, w0=w0, w1=w1: _il_gpu_module(d, True, w0, w1, False), scalars=["loss"], caps=IL_CAPS, margin=margin))
        for nblk in (1, 64, 1024):
            out.append(KCase("image_loss", f"{sh}-raw-nblk{nblk}", make, lambda d: _il_ref(d, True, 1.0, 0.5),
                             lambda d, nblk=nblk: _il_gpu_raw(d, True, 1.0, 0.5, nblk), scalars=["loss"], caps=IL_CAPS, margin=margin))
        out.append(KCase("image_loss", f"{sh}-module-gradient-off", make, lambda d: _il_ref(d, False, 20.0, 1e-4),
                         lambda d: _il_gpu_module(d, False, 20.0, 1e-4, False), scalars=["loss"], caps=IL_CAPS))
        out.append(KCase("image_loss", f"{sh}-raw-gradient-off-nblk64", make, lambda d: _il_ref(d, False, 1.0, 0.5),
                         lambda d: _il_gpu_raw(d, False, 1.0, 0.5, 64), scalars=["loss"], caps=IL_CAPS))
        if shape[1] <= 3:
            out.append(KCase("gradient_prior_loss", sh, make, lambda d: _il_ref(d, True, 0.0, 1.0), lambda d: _il_gpu_module(d, True, 0.0, 1.0, True),
                             scalars=["loss"], caps=IL_CAPS, margin=margin))
        else:
            out.append(KCase("gradient_prior_loss", f"{sh}-raw-w0-zero", make, lambda d: _il_ref(d, True, 0.0, 1.0), lambda d: _il_gpu_raw(d, True, 0.0, 1.0, 64),
                             scalars=["loss"], caps=IL_CAPS, margin=margin))
    return out


def _margin(value, what, m=MARGIN):
    assert value >= m, f"{what}: margin {value:.3e} < {m:.0e}"


# ---- softmax + semantic loss + prior ------------------------------------------------------------------------------------------
def _away_from(q, p, m=2 * MARGIN):
    """q (fp32) where it is closer than m to p (fp64): p + 2 m"""
    return torch.where((q.double() - p).abs() < m, p + 2 * m, q.double()).float()


def _sp_make(N, T, C, kind, seed):
    g = _gen("softmax_prior", N, T, C, kind, seed)
    x = torch.randn(N, T, C, generator=g) * 2
    if kind == "saturated":          # row 0 mod 3: one class 200 above the rest (p underflows to 0 in float32), row 1 mod 3: 30 above (p ~ 1e-13)
        rows = x.view(-1, C)
        hot = torch.randint(0, C, (rows.shape[0],), generator=g)
        lift = torch.tensor([200.0, 30.0, 0.0])[torch.arange(rows.shape[0]) % 3]
        rows[torch.arange(rows.shape[0]), hot] += lift
    p = torch.softmax(x.double(), -1)
    q = torch.softmax(torch.randn(N, T, C, generator=g) * 2, -1) if C > 1 else torch.rand(N, T, C, generator=g) * 0.8
    if kind == "saturated":
        q = q * 0.5 + 0.01           # away from the 0 / 1 the saturated p sits at
    return {"logits": x, "q": _away_from(q, p), "dprior": torch.randn(N, C, 1, T, generator=g), "dp_in": torch.randn(N, T, C, generator=g)}


def _sp_ref(d, drop_n, w, use):
    x = d["logits"].clone().requires_grad_(True)
    N = x.shape[0]
    p = torch.softmax(x, -1)
    res = {"p": p}
    tot = 0
    if "q" in use:
        q = d["q"]
        loss = w * ((q - p).abs().mean() + ((q + 1e-20) * (torch.log(q + 1e-20) - torch.log(p + 1e-20))).mean())
        res["loss"] = loss.reshape(())
        tot = tot + loss
    keep = (torch.arange(N) >= drop_n).to(x.dtype).view(N, 1, 1, 1)
    prior = p.permute(0, 2, 1).unsqueeze(2) * keep
    res["prior"] = prior
    if "dprior" in use:
        tot = tot + (prior * d["dprior"]).sum()
    if "dp_in" in use:
        tot = tot + (p * d["dp_in"]).sum()
    tot.backward()
    res["dlogits"] = x.grad
    return res


def _sp_gpu(d, drop_n, w, use, nblk):
    k = K()
    x = d["logits"]
    N, T, C = x.shape
    q = d["q"] if "q" in use else None
    p, prior, dl = (torch.full(s, float("nan"), device=DEV) for s in ((N, T, C), (N, C, 1, T), (N, T, C)))
    part = torch.full((nblk, 2), float("nan"), device=DEV)
    loss = torch.full((1,), float("nan"), device=DEV)
    k.softmax_prior_fwd(x, q, N, T, C, drop_n, p, prior, part, nblk)
    res = {"p": p, "prior": prior}
    if q is not None:
        k.semantic_loss_finalize(part, nblk, N * T * C, w, loss)
        res["loss"] = loss.reshape(())
    k.softmax_prior_bwd(p, q, d["dprior"] if "dprior" in use else None, d["dp_in"] if "dp_in" in use else None, N, T, C, drop_n, w, dl, nblk)
    torch.cuda.synchronize()
    want = p.permute(0, 2, 1).unsqueeze(2).clone()
    want[:drop_n] = 0
    assert torch.equal(prior, want), "the prior is not the kernel's own p, transposed, with the first drop_n samples zeroed"
    res["dlogits"] = dl
    return res


SOFTMAX_PRIOR = [
    # name, N, T, C, kind, drop_n, w, what the backward receives, nblk                 rows = N T
    ("C37-rows78-nblk8", 3, 26, 37, "plain", 1, 100.0, ("q", "dprior"), 8),
    ("C37-rows78-nblk1", 3, 26, 37, "plain", 0, 1.0, ("q", "dprior", "dp_in"), 1),
    ("C37-rows78-nblk64-few-rows", 3, 26, 37, "plain", 3, 100.0, ("q", "dprior"), 64),
    ("C37-rows7-nblk3", 1, 7, 37, "plain", 0, 1.0, ("q", "dp_in"), 3),
    ("C37-no-q", 4, 26, 37, "plain", 2, 1.0, ("dprior",), 8),
    ("C37-no-q-dp_in-only", 2, 5, 37, "plain", 1, 1.0, ("dp_in",), 2),
    ("C1", 2, 5, 1, "plain", 1, 1.0, ("q", "dprior", "dp_in"), 2),
    ("C64", 2, 9, 64, "plain", 1, 100.0, ("q", "dprior"), 4),
    ("C63", 2, 9, 63, "plain", 0, 100.0, ("q", "dprior", "dp_in"), 4),
    ("C37-saturated", 3, 26, 37, "saturated", 1, 100.0, ("q", "dprior"), 8),
    ("C64-saturated", 2, 11, 64, "saturated", 0, 1.0, ("q", "dprior", "dp_in"), 64),
    ("C37-rows1248-grid-stride", 48, 26, 37, "plain", 12, 100.0, ("q", "dprior"), 8),
]


def _sem_make(shape, scale, seed):
    g = _gen("semantic_loss", shape, scale, seed)
    p = torch.softmax(torch.randn(*shape, generator=g) * 2, -1) * scale
    q = torch.softmax(torch.randn(*shape, generator=g) * 2, -1)
    return {"p": p, "q": _away_from(q, p.double()), "up": torch.rand(1, generator=g) * 4 + 1}


def _sem_ref(d):
    p, q = d["p"].clone().requires_grad_(True), d["q"]
    loss = (q - p).abs().mean() + ((q + 1e-20) * (torch.log(q + 1e-20) - torch.log(p + 1e-20))).mean()
    (loss * d["up"][0]).backward()
    return {"loss": loss.detach().reshape(()), "dp": p.grad}


def _sem_gpu(d):
    from tpgsr_amd.loss.semantic_loss import SemanticLoss
    p = d["p"].clone().requires_grad_(True)
    loss = SemanticLoss()(p, d["q"])
    (loss * d["up"][0]).backward()
    return {"loss": loss.detach().reshape(()), "dp": p.grad}


def _semantic_cases():
    out = []
    for name, N, T, C, kind, drop_n, w, use, nblk in SOFTMAX_PRIOR:
        margin = (lambda d64: _margin((d64["q"] - torch.softmax(d64["logits"], -1)).abs().min().item(), "|q - p|")) if "q" in use else None
        out.append(KCase("softmax_prior", name, lambda seed, a=(N, T, C, kind): _sp_make(*a, seed), lambda d, a=(drop_n, w, use): _sp_ref(d, *a),
                         lambda d, a=(drop_n, w, use, nblk): _sp_gpu(d, *a), scalars=["loss"] if "q" in use else [], margin=margin))
    for shape, scale in [((26, 3, 37), 1.0), ((26, 3, 37), 0.7), ((1, 1, 5), 1.0), ((26, 32, 37), 1.0), ((3, 2, 1), 0.6)]:
        out.append(KCase("semantic_loss", f"{'x'.join(map(str, shape))}-scale{scale:g}", lambda seed, a=(shape, scale): _sem_make(*a, seed), _sem_ref, _sem_gpu,
                         scalars=["loss"], caps={"loss": 2e-6, "dp": 1e-5}, margin=lambda d64: _margin((d64["q"] - d64["p"]).abs().min().item(), "|q - p|")))
    return out


# ---- CTC -------------------------------------------------------------------------------------------------------------------
CTC = [
    # name, T, C, blank, labels of every sample, weight, accumulate
    ("T26-C37", 26, 37, 0, [[], [5], [1, 2, 3], [7, 7], [3, 0, 4], list(range(1, 16)), [9, 9, 9, 2, 2], [8, 5, 12, 12, 15, 23, 15, 18, 12, 4, 4, 1, 36, 36, 2]], True, True),
    ("T32-C37-S63-and-tight-repeats", 32, 37, 0, [list(range(1, 32)), [1, 2] * 15 + [1], [1] * 13 + [2, 3, 4, 5, 6, 7, 8], [4] * 16, []], False, False),
    ("T32-C64-blank63", 32, 64, 63, [[(7 * i) % 63 for i in range(31)], [0, 62, 0, 62, 5, 5, 5, 61, 1, 2], [], [62]], True, False),
    ("T1-C37", 1, 37, 0, [[], [4], []], True, True),
    ("T5-C1", 5, 1, 0, [[], []], False, False),
    ("T12-C10-blank5", 12, 10, 5, [[1, 2, 3], [6, 6, 4], [0, 9], [], [5, 1, 2]], True, False),
]


def _ctc_feasible(T, labels):
    return all(len(l) + sum(a == b for a, b in zip(l, l[1:])) <= T for l in labels)


def _ctc_make(T, C, labels, seed):
    g = _gen("ctc", T, C, len(labels), seed)
    N = len(labels)
    return {"x": torch.randn(T, N, C, generator=g) * 2, "weight": torch.rand(N, generator=g) + 0.5, "pre": torch.randn(T, N, C, generator=g)}


def _ctc_ref(d, labels, blank, weighted, accumulate, scale):
    x = d["x"].clone().requires_grad_(True)
    T, N, C = x.shape
    tg = torch.tensor([v for l in labels for v in l], dtype=torch.long)
    nll = F.ctc_loss(torch.log_softmax(x, -1), tg, torch.full((N,), T, dtype=torch.long), torch.tensor([len(l) for l in labels], dtype=torch.long),
                     blank=blank, reduction="none", zero_infinity=False)
    w = d["weight"] if weighted else torch.ones_like(d["weight"])
    (scale * w * nll).sum().backward()
    return {"nll": nll.detach(), "dlogits": x.grad + d["pre"] if accumulate else x.grad}


def _ctc_operands(labels):
    lens = torch.tensor([len(l) for l in labels], dtype=torch.int32)
    off = torch.zeros_like(lens)
    off[1:] = torch.cumsum(lens, 0)[:-1]
    tg = torch.tensor([v for l in labels for v in l] + [0], dtype=torch.int32)      # (one spare element: an empty batch still has an address)
    return tg.to(DEV), off.to(DEV), lens.to(DEV), int(lens.max())


def _ctc_gpu(d, labels, blank, weighted, accumulate, scale, layout):
    k = K()
    T, N, C = d["x"].shape
    tg, off, lens, mx = _ctc_operands(labels)
    if layout == "TNC":
        x, dl, sn, st = d["x"], d["pre"].clone(), C, N * C
    else:
        x, dl, sn, st = d["x"].permute(1, 0, 2).contiguous(), d["pre"].permute(1, 0, 2).contiguous(), T * C, C
    if not accumulate:
        dl.fill_(float("nan"))
    nll = torch.full((N,), float("nan"), device=DEV)
    k.ctc_loss(x, sn, st, tg, off, lens, d["weight"] if weighted else None, N, T, C, blank, scale, nll, dl, accumulate, mx)
    nll2 = torch.full((N,), float("nan"), device=DEV)
    k.ctc_loss(x, sn, st, tg, off, lens, None, N, T, C, blank, 0.0, nll2, None, False, mx)      # the value-only call: the same numbers
    torch.cuda.synchronize()
    assert torch.equal(nll, nll2)
    return {"nll": nll, "dlogits": dl if layout == "TNC" else dl.permute(1, 0, 2)}


def _ctc_cases():
    out = []
    for name, T, C, blank, labels, weighted, accumulate in CTC:
        scale = 1.0 / len(labels)
        for layout in ("TNC", "NTC"):
            out.append(KCase("ctc_loss", f"{name}-{layout}", lambda seed, a=(T, C, labels): _ctc_make(*a, seed),
                             lambda d, a=(labels, blank, weighted, accumulate, scale): _ctc_ref(d, *a),
                             lambda d, a=(labels, blank, weighted, accumulate, scale, layout): _ctc_gpu(d, *a),
                             scalars=["nll"], caps={"nll": 2e-6, "dlogits": 4e-5}))
    return out


_CASES = None


def all_cases():
    global _CASES
    if _CASES is None:
        _CASES = _image_cases() + _semantic_cases() + _ctc_cases()
        ids = [c.id for c in _CASES]
        assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return _CASES


# ---- optimiser: its own table (a trajectory, compared after every step) ---------------------------------------------------------------
STRIDE2 = 2 * 256 * 4          # floats one block consumes per trip of sumsq_partial's two-loads-in-flight loop
OPT = [
    # name, n, nblk, max_norm, gradient std, mode, steps, zero gradients in the first third
    #   inc: sumsq, clip_coef, step_inc, adam(coef)      steps1 / steps8 / steps0: clip_coef_steps with that many counters (steps0: + step_inc)
    #   noclip: clip_coef_steps(partial=None) + adam(gscale=None)      scale: sumsq, clip_coef, scale_(g), step_inc, adam(gscale=None)
    ("n1", 1, 1, 0.25, 3.0, "inc", 20, False),
    ("n2", 2, 4, 0.25, 3.0, "steps1", 20, False),
    ("n3", 3, 1, 0.25, 3.0, "steps8", 20, False),
    ("n4", 4, 2, 0.25, 3.0, "inc", 20, False),
    ("n5", 5, 128, 0.25, 3.0, "steps0", 20, False),
    ("n7-not-clipping", 7, 1, 1e6, 1.0, "steps1", 20, False),
    ("n1023-scale", 1023, 2, 0.25, 3.0, "scale", 20, False),
    ("n4095-one-trip-minus-1", 2 * STRIDE2 - 1, 2, 0.25, 3.0, "inc", 20, False),
    ("n4096-one-trip", 2 * STRIDE2, 2, 0.25, 3.0, "steps1", 20, False),
    ("n4097-one-trip-plus-1-not-clipping", 2 * STRIDE2 + 1, 2, 1e6, 0.01, "inc", 20, False),
    ("n4101-one-trip-plus-5", 2 * STRIDE2 + 5, 2, 0.25, 3.0, "steps8", 20, False),
    ("n2054-second-load-ragged", STRIDE2 + 6, 1, 0.25, 3.0, "inc", 20, False),
    ("n100003-zero-gradients", 100003, 128, 0.25, 3.0, "steps1", 24, True),
    ("n100003-noclip", 100003, 128, 0.0, 0.02, "noclip", 24, False),
    ("n100003-scale-not-clipping", 100003, 256, 50.0, 0.05, "scale", 20, False),
    ("n3000001-nblk1024", 3000001, 1024, 0.25, 1.0, "steps1", 20, False),
    ("n4194311-nblk1024-two-trips", 2 * STRIDE2 * 1024 + 7, 1024, 0.25, 1.0, "inc", 20, True),
]


def _opt_grad(name, n, std, zeros, t, seed=0):
    g = torch.randn(n, generator=_gen("opt-grad", name, t, seed)) * std
    if zeros:
        g[: n // 3] = 0.0
    return g


class _TorchTrajectory:
    """clip_grad_norm_ + torch.optim.Adam on one flat parameter, in `dtype`"""

    def __init__(self, p0, dtype, max_norm, clip):
        self.p = torch.nn.Parameter(p0.to(dtype).clone())
        self.opt = torch.optim.Adam([self.p], lr=1e-3, betas=(0.5, 0.999), eps=1e-8)
        self.max_norm, self.clip = max_norm, clip

    def step(self, g):
        self.p.grad = g.to(self.p.dtype).clone()
        res = {}
        if self.clip:
            norm = torch.nn.utils.clip_grad_norm_([self.p], self.max_norm)
            res["norm"] = norm.detach().reshape(())
            res["coef"] = torch.clamp(self.max_norm / (norm.detach() + 1e-6), max=1.0).reshape(())
            res["g"] = self.p.grad.detach().clone()
        self.opt.step()
        st = self.opt.state[self.p]
        res.update(p=self.p.detach(), m=st["exp_avg"], v=st["exp_avg_sq"])
        return res


def _norm_e32(grads, max_norm):
    """scalars rule for the norm and the clip coefficient: the worst float32-CPU error over the given gradients"""
    e = {"norm": 0.0, "coef": 0.0}
    for g in grads:
        r = {}
        for dt in (F64, torch.float32):
            q = torch.nn.Parameter(torch.zeros(g.numel(), dtype=dt))
            q.grad = g.to(dt)
            n = torch.nn.utils.clip_grad_norm_([q], max_norm).detach()
            r[dt] = (n, torch.clamp(max_norm / (n + 1e-6), max=1.0))
        e["norm"] = max(e["norm"], err(r[torch.float32][0], r[F64][0]))
        e["coef"] = max(e["coef"], err(r[torch.float32][1], r[F64][1]))
    return e


# adam_step_kernel takes beta2 as a float and forms (1.f - beta2) in float32: beta2 = 0.999 is rounded by up to 2^-25 on the way in, which is
# 2^-25 / (1 - beta2) = 3.0e-5 of the factor of g^2 (here: 1 - 0.999f = 0.00099998713, 1.3e-5 below 0.001), where torch.optim.Adam takes
# 1 - beta2 from the Python double.  v carries that relative offset (sqrt(v): half of it; p, after bias correction by the exact 1 - beta2^t,
# moves by ~6e-6 of one update, 6e-9 absolute: inside its own bound).  beta1 = 0.5 is exact, m has no such term.
V_BETA2_TERM = 2.0 ** -25 / (1 - 0.999)


def _opt_compare(tag, got, r64, r32, e_scalar, worst, fam):
    for key in sorted(r64):
        if key in ("norm", "coef"):
            e32 = e_scalar[key]
        else:
            e32 = err(r32[key], r64[key])
        bound = 4 * e32 + FLOOR
        if key == "norm":
            bound = min(bound, 1e-4)
        if key == "v":
            bound += V_BETA2_TERM
        e_gpu = err(got[key].cpu(), r64[key])
        worst[fam] = max(worst.get(fam, 0.0), e_gpu / bound)
        print(f"{tag} {key}: e_gpu {e_gpu:.2e}  e_ref32 {e32:.2e}  bound {bound:.2e}  ratio {e_gpu / bound:.2f}")
        assert e_gpu <= bound, f"{tag} {key}: e_gpu {e_gpu:.3e} > {bound:.3e} (e_ref32 {e32:.3e})"
        if key == "p":
            a = (got[key].cpu().double() - r64[key]).abs().max().item()
            assert a <= 2e-6, f"{tag} p: max |got - ref64| {a:.3e} > 2e-6"


def _opt_params():
    return [pytest.param(c, id=c[0], marks=pytest.mark.gpu) for c in OPT]


# ---- CPU: the tables are well posed ---------------------------------------------------------------------------------------------
def test_case_table_is_well_posed():
    """Every case on the CPU: margins from the L1 kinks, a finite float64 reference that gives every output and gradient, a finite e_ref32 (over
    8 seeds for the scalars), inputs under 8 MB; every CTC target feasible and inside the kernel's contract; the optimiser table's sizes sit
    where its comments say; the families cover every kernel the table of the issue names."""
    cases = all_cases()
    fams = {c.family for c in cases} | {"optimiser", "fused_adam"}
    assert fams == set(FAMILY_KERNELS)
    assert set().union(*FAMILY_KERNELS.values()) >= NAMED_IN_THE_ISSUE
    for c in cases:
        check_well_posed(c)
    for name, T, C, blank, labels, _w, _a in CTC:
        assert T <= 32 and C <= 64 and 0 <= blank < C and all(len(l) <= 31 and all(0 <= v < C for v in l) for l in labels), name
        assert _ctc_feasible(T, labels), name
    assert any(len(l) == 31 and T == 32 for _n, T, _C, _b, ls, _w, _a in CTC for l in ls)                       # S = 63: the last lane pair
    assert any(len(l) and len(l) + sum(a == b for a, b in zip(l, l[1:])) == T for _n, T, _C, _b, ls, _w, _a in CTC for l in ls)     # tightly feasible
    assert any(blank in l for _n, _T, _C, blank, ls, _w, _a in CTC for l in ls)                                  # a label with the blank's index
    big = 0
    for name, n, nblk, max_norm, std, mode, steps, zeros in OPT:
        assert steps >= 20 and mode in ("inc", "steps1", "steps8", "steps0", "noclip", "scale"), name
        big += n * 4 >= 8 << 20
        g = _opt_grad(name, n, std, zeros, 1)
        norm = g.double().norm().item()
        if "not-clipping" in name:
            assert norm < max_norm
        elif mode != "noclip":
            assert norm > 2 * max_norm, (name, norm)
        e = _norm_e32([_opt_grad(name, n, std, zeros, 1, s) for s in range(8)] if n < 1 << 20 else [g], max_norm if mode != "noclip" else 1.0)
        assert all(math.isfinite(v) for v in e.values())
    assert big == 2 and {c[1] & 3 for c in OPT} == {0, 1, 2, 3}
    # a short trajectory of the reference in both precisions: finite, and the float32 one stays inside the absolute cap on its own
    t64, t32 = _TorchTrajectory(torch.ones(5), F64, 0.25, True), _TorchTrajectory(torch.ones(5), torch.float32, 0.25, True)
    for t in range(1, 21):
        g = _opt_grad("wp", 5, 3.0, False, t)
        a, b = t64.step(g), t32.step(g)
        assert all(torch.isfinite(a[k]).all() for k in a) and (a["p"] - b["p"].double()).abs().max() < 2e-6


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
WORST = {}


@pytest.mark.parametrize("case", [pytest.param(c, id=c.id, marks=pytest.mark.gpu) for c in all_cases()])
def test_kernel_vs_fp64(case):
    check_case(case, WORST)


@pytest.mark.parametrize("spec", _opt_params())
def test_clip_and_adam_trajectory(spec):
    """raw kernels over one flat arena: norm, clip coefficient, (scaled gradient,) p, m, v and the step counters after every step"""
    name, n, nblk, max_norm, std, mode, steps, zeros = spec
    k = K()
    clip = mode != "noclip"
    p0 = torch.randn(n, generator=_gen("opt-p0", name))
    t64, t32 = _TorchTrajectory(p0, F64, max_norm, clip), _TorchTrajectory(p0, torch.float32, max_norm, clip)
    e_scalar = _norm_e32([_opt_grad(name, n, std, zeros, 1, s) for s in range(8)], max_norm) if clip else {}
    pd, m, v = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    extra = [torch.full((1,), 100 * (i + 1), dtype=torch.int32, device=DEV) for i in range(7)]
    part = torch.full((nblk,), float("nan"), device=DEV)
    coef, nrm = torch.full((1,), float("nan"), device=DEV), torch.full((1,), float("nan"), device=DEV)
    for t in range(1, steps + 1):
        g = _opt_grad(name, n, std, zeros, t)
        r64, r32 = t64.step(g), t32.step(g)
        gd = g.to(DEV)
        got = {}
        if clip:
            k.sumsq_partial(gd, n, part, nblk)
        if mode == "inc" or mode == "scale":
            k.clip_coef(part, nblk, max_norm, coef, nrm)
            if mode == "scale":
                k.scale_(gd, n, coef)
            k.step_inc(step)
        elif mode == "steps1":
            k.clip_coef_steps(part, nblk, max_norm, coef, nrm, [step])
        elif mode == "steps8":
            k.clip_coef_steps(part, nblk, max_norm, coef, nrm, extra[:3] + [step] + extra[3:])
        elif mode == "steps0":
            k.clip_coef_steps(part, nblk, max_norm, coef, nrm, [])
            k.step_inc(step)
        else:
            k.clip_coef_steps(None, 0, 0.0, None, None, [step])
        k.adam_step(pd, gd, m, v, n, coef if mode in ("inc", "steps1", "steps8", "steps0") else None, 1e-3, 0.5, 0.999, 1e-8, step)
        torch.cuda.synchronize()
        assert int(step.item()) == t
        if mode == "steps8":
            assert [int(x.item()) for x in extra] == [100 * (i + 1) + t for i in range(7)]
        if clip:
            got.update(norm=nrm.reshape(()), coef=coef.reshape(()))
            if mode == "scale":
                got["g"] = gd
            else:
                del r64["g"], r32["g"]
        got.update(p=pd, m=m, v=v)
        _opt_compare(f"optimiser-{name} step {t}", got, r64, r32, e_scalar, WORST, "optimiser")


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["unclipped-first", "clipped-first"])
def test_fused_adam_step_on_two_modules(order):
    """FusedAdam.step() itself on two small TSRN networks, one clipped and one not, 22 steps on random gradients written into the arenas:
    unclipped-first makes the step open with clip_coef_steps(partial=None) (all counters) and clip the second module with clip_coef;
    clipped-first puts the clip and both counters into one clip_coef_steps launch.  Flat parameters, both moments, the counters, the
    clipped module's norm and coefficient against clip_grad_norm_ + torch.optim.Adam in float64 after every step."""
    from tpgsr_amd.model import tsrn
    from tpgsr_amd.optim import FusedAdam
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(5)
        sr, other = tsrn.TSRN(srb_nums=1, mask=True).to(DEV), tsrn.TSRN(srb_nums=1, mask=False).to(DEV)
    mods = [other, sr] if order == "unclipped-first" else [sr, other]
    opt = FusedAdam(mods, lr=1e-3, betas=(0.5, 0.999), clip_modules=[sr], max_norm=0.25)
    arenas = {id(m): opt._st(m)[0] for m in mods}
    traj, e_scalar = {}, {}
    for m in mods:
        a = arenas[id(m)]
        assert all(a.flat.data_ptr() <= p.data_ptr() < a.flat.data_ptr() + 4 * a.numel for p in m.parameters())      # the module's parameters ARE the arena
        p0 = a.flat.detach().cpu().clone()
        traj[id(m)] = (_TorchTrajectory(p0, F64, 0.25, m is sr), _TorchTrajectory(p0, torch.float32, 0.25, m is sr))
    e_scalar = _norm_e32([_opt_grad("fused-sr", arenas[id(sr)].numel, 0.05, False, 1, s) for s in range(8)], 0.25)
    for t in range(1, 23):
        grads = {}
        for m in mods:
            a = arenas[id(m)]
            grads[id(m)] = _opt_grad("fused-sr" if m is sr else "fused-other", a.numel, 0.05, False, t)
            a.grad.copy_(grads[id(m)].to(DEV))
        opt.step()
        torch.cuda.synchronize()
        for m in mods:
            a, st = arenas[id(m)], opt.state[id(m)]
            r64, r32 = (tr.step(grads[id(m)]) for tr in traj[id(m)])
            assert int(st["step"].item()) == t
            got = dict(p=a.flat.detach(), m=st["m"], v=st["v"])
            if m is sr:
                got.update(norm=opt.grad_norm(m).reshape(()), coef=st["coef"].reshape(()))
                assert r64["coef"].item() < 1.0
                del r64["g"], r32["g"]
            else:
                assert st["coef"].item() == 1.0 and st["norm"].item() == 0.0
            _opt_compare(f"fused_adam-{order}-{'sr' if m is sr else 'other'} step {t}", got, r64, r32, e_scalar, WORST, "fused_adam")


@pytest.mark.gpu
def test_l1_terms_with_sign_zero_have_no_gradient():
    """exact zeros: a 1x1 image (every neighbour of gradmag is padding: both maps are sqrt(1e-6), their difference is exactly 0), out == tgt on a
    larger one, q == p in both semantic-loss backward kernels: the L1 term contributes exactly nothing, what is left is the MSE / KL term"""
    k = K()
    g = _gen("sign-zero")
    for shape in [(3, 4, 1, 1), (2, 3, 1, 1)]:
        out, tgt = torch.randn(*shape, generator=g), torch.randn(*shape, generator=g)
        N, C, H, W = shape
        dl, dout = torch.tensor([1.7], device=DEV), torch.empty(*shape, device=DEV)
        part, loss = torch.empty(64, 2, device=DEV), torch.empty(1, device=DEV)
        k.image_loss_fwd(out.to(DEV), tgt.to(DEV), N, C, H, W, True, part, 64)
        k.image_loss_finalize(part, 64, out.numel(), N * min(C, 3) * H * W, 1.0, 0.5, loss)
        k.image_loss_bwd(out.to(DEV), tgt.to(DEV), dl, N, C, H, W, True, 1.0, 0.5, dout)
        torch.cuda.synchronize()
        ref = 1.7 * 2 * (out.double() - tgt.double()) / out.numel()
        assert err(dout.cpu(), ref) <= FLOOR
        assert abs(loss.item() - ((out.double() - tgt.double()) ** 2).mean().item()) <= 1e-6 * max(1.0, loss.item())
    x = torch.randn(2, 4, 6, 9, generator=g).to(DEV)
    dout = torch.full_like(x, float("nan"))
    k.image_loss_bwd(x, x.clone(), torch.ones(1, device=DEV), 2, 4, 6, 9, True, 1.0, 0.5, dout)
    torch.cuda.synchronize()
    assert torch.equal(dout, torch.zeros_like(dout))
    # q == p: d logits of the fused kernel is softmax-backward of the KL term alone, -w / count * q' / p' = -w / count per element => exactly
    # p * (dp - sum(p dp)); against float64 with the L1 sign taken as 0
    N, T, C = 2, 5, 37
    lg = (torch.randn(N, T, C, generator=g) * 2).to(DEV)
    p, prior, part = torch.empty(N, T, C, device=DEV), torch.empty(N, C, 1, T, device=DEV), torch.empty(4, 2, device=DEV)
    k.softmax_prior_fwd(lg, None, N, T, C, 0, p, prior, part, 4)
    dlg, dp = torch.empty(N, T, C, device=DEV), torch.empty(N, T, C, device=DEV)
    k.softmax_prior_bwd(p, p.clone(), None, None, N, T, C, 0, 100.0, dlg, 4)
    k.semantic_loss_bwd(p, p.clone(), torch.tensor([3.0], device=DEV), p.numel(), dp)
    torch.cuda.synchronize()
    p64 = p.cpu().double()
    d = -100.0 / p.numel() * (p64 + 1e-20) / (p64 + 1e-20)
    ref = p64 * (d - (p64 * d).sum(-1, keepdim=True))
    assert (dlg.cpu().double() - ref).abs().max().item() <= 4 * 2.0 ** -24 * 100.0 / p.numel()
    assert err(dp.cpu(), torch.full((N, T, C), -3.0 / p.numel(), dtype=F64)) <= FLOOR


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["TNC", "NTC"])
def test_ctc_infeasible_target(layout):
    """labels 1 1 2 at T = 3 need four steps.  Pinned: nll = +inf (as ATen); the gradient of that sample is the FINITE scale * weight * softmax(x)
    (ATen with zero_infinity=False gives NaN there -- the module docstring says why the kernel does not); every other sample's nll and gradient
    are bit-identical to the same batch without the infeasible sample."""
    k = K()
    T, C = 3, 10
    labels = [[4, 5], [1, 1, 2], [], [3]]
    assert not _ctc_feasible(T, labels) and _ctc_feasible(T, [labels[0], labels[2], labels[3]])
    d = _ctc_make(T, C, labels, 0)
    ref = torch.nn.functional.ctc_loss(torch.log_softmax(d["x"].double(), -1), torch.tensor([4, 5, 1, 1, 2, 3]), torch.full((4,), T), torch.tensor([2, 3, 0, 1]),
                                       blank=0, reduction="none")
    assert torch.isinf(ref[1]) and ref[1] > 0 and torch.isfinite(ref[[0, 2, 3]]).all()

    def run(keep):
        x, w = d["x"][:, keep].contiguous(), d["weight"][keep].contiguous().to(DEV)
        ls = [labels[i] for i in keep]
        N = len(keep)
        tg, off, lens, mx = _ctc_operands(ls)
        xd = (x if layout == "TNC" else x.permute(1, 0, 2).contiguous()).to(DEV)
        sn, st = (C, N * C) if layout == "TNC" else (T * C, C)
        nll, dl = torch.full((N,), float("nan"), device=DEV), torch.full_like(xd, float("nan"))
        k.ctc_loss(xd, sn, st, tg, off, lens, w, N, T, C, 0, 0.25, nll, dl, False, mx)
        torch.cuda.synchronize()
        return nll.cpu(), (dl if layout == "TNC" else dl.permute(1, 0, 2)).cpu()
    nll, dl = run([0, 1, 2, 3])
    nll3, dl3 = run([0, 2, 3])
    assert nll[1].item() == float("inf")
    assert torch.equal(nll[[0, 2, 3]], nll3) and torch.equal(dl[:, [0, 2, 3]], dl3)
    want = 0.25 * d["weight"][1].double() * torch.softmax(d["x"][:, 1].double(), -1)
    assert torch.isfinite(dl[:, 1]).all() and err(dl[:, 1], want) <= FLOOR + 4 * err(0.25 * d["weight"][1] * torch.softmax(d["x"][:, 1], -1), want)
    assert err(nll3, ref[[0, 2, 3]]) <= 2e-6


@pytest.mark.gpu
def test_ctc_last_label_with_the_blanks_index():
    """labels 5 1 5 with blank = 5: the last label carries the blank's index, so the two final states of l' belong to the same class.  ATen's
    CPU backward ASSIGNS the class's occupancy at t = T - 1 twice (once per final state) instead of adding the two, so its analytic gradient at
    (T - 1, blank) is not the derivative of its own (correct) nll; the kernel adds them.  The reference here is therefore the central
    difference of F.ctc_loss's float64 VALUE (step 1e-6, error ~1e-10), every element of the sample, under the fixture test's 4e-5."""
    k = K()
    T, C, blank, labels = 12, 10, 5, [[5, 1, 5], [2, 5]]
    x = _ctc_make(T, C, labels, 0)["x"]

    def nll64(xx):
        return F.ctc_loss(torch.log_softmax(xx, -1), torch.tensor([5, 1, 5, 2, 5]), torch.full((2,), T), torch.tensor([3, 2]), blank=blank, reduction="none")
    x64 = x.double()
    fd = torch.zeros(T, 2, C, dtype=F64)
    for t in range(T):
        for c in range(C):
            e = torch.zeros_like(x64)
            e[t, :, c] = 1e-6
            fd[t, :, c] = (nll64(x64 + e) - nll64(x64 - e)) / 2e-6
    xr = x64.clone().requires_grad_(True)
    nll64(xr).sum().backward()
    print(f"ATen's analytic gradient against the central difference of its own value: {err(xr.grad, fd):.2e}")
    tg, off, lens, mx = _ctc_operands(labels)
    nll, dl = torch.full((2,), float("nan"), device=DEV), torch.full((T, 2, C), float("nan"), device=DEV)
    k.ctc_loss(x.to(DEV), C, 2 * C, tg, off, lens, None, 2, T, C, blank, 1.0, nll, dl, False, mx)
    torch.cuda.synchronize()
    e_n, e_d = err(nll.cpu(), nll64(x64)), err(dl.cpu(), fd)
    print(f"kernel: nll {e_n:.2e}, gradient against the central difference {e_d:.2e}")
    assert e_n <= 2e-6 and e_d <= 4e-5


@pytest.mark.gpu
def test_argument_guards():
    """just past each limit of the contract: the library's own error, before any launch"""
    from tpgsr_amd._lib import TpgsrKernelError
    k = K()
    x = torch.zeros(33 * 2 * 65, device=DEV)
    i32 = torch.zeros(4, dtype=torch.int32, device=DEV)
    nll = torch.zeros(2, device=DEV)
    for T, C, mx in [(33, 37, 15), (32, 65, 15), (32, 37, 32)]:
        with pytest.raises(TpgsrKernelError, match="T <= 32, C <= 64, at most 31 labels"):
            k.ctc_loss(x, C, 2 * C, i32, i32, i32, None, 2, T, C, 0, 1.0, nll, None, False, mx)
    with pytest.raises(TpgsrKernelError, match="blank|T <= 32"):
        k.ctc_loss(x, 37, 74, i32, i32, i32, None, 2, 26, 37, 37, 1.0, nll, None, False, 15)
    with pytest.raises(TpgsrKernelError, match="C <= 64"):
        k.softmax_prior_fwd(x, None, 2, 3, 65, 0, x.clone(), None, None, 4)
    with pytest.raises(TpgsrKernelError, match="16-byte aligned"):
        k.sumsq_partial(x[1:], 8, nll, 2)
    with pytest.raises(TpgsrKernelError, match="at most eight step counters"):
        k.clip_coef_steps(None, 0, 0.0, None, None, [torch.zeros(1, dtype=torch.int32, device=DEV) for _ in range(9)])
    with pytest.raises(TpgsrKernelError, match="distinct"):
        k.clip_coef_steps(None, 0, 0.0, None, None, [i32, i32])
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_zz_report_worst_ratios():
    """prints the worst e_gpu / bound per family seen by this run (the module docstring's observed lines are a copy of it)"""
    for fam in sorted(WORST):
        print(f"worst e_gpu / bound  {fam:24s} {WORST[fam]:.3f}")
