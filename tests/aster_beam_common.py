"""shared by the ASTER beam-search tests and tests/golden/make_golden_aster_beam.py: a restatement of the reference's
AttentionRecognitionHead.beam_search (attention_recognition_head.py:68-184) in any floating dtype (the tests use float64), the fixture, the
fixture's weights, and the fixture's conditions (finite scores, selection margin, coverage) recomputed from stored histories.

Layout: N images, B beams, C classes, L steps, row r = n * B + b.  Where torch.topk leaves the order of equal values open it is fixed
here: higher value first, then LOWER index; a NaN counts as -inf; -inf candidates are taken in index order once the finite ones run out."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE, GOLDEN):
    if _p not in sys.path:
        sys.path.insert(0, _p)

GAP = 1e-3                # the fixture's selection margin g
SCORE_TOL = GAP / 8       # a decision flips only if two scores together move by g: g / 8 per score leaves a fourfold margin
NINF = float("-inf")


def fixture():
    return np.load(os.path.join(GOLDEN, "aster_beam.npz"))


def beam_state_dict(seed: int, eos: int, eos_bias: float):
    """the fixture's weights: make_golden_aster's recipe (generic recipe, classifier x 40) + `eos_bias` on the classifier's eos
    bias, which is what makes sequences end (and several end together) within a dozen steps"""
    from aster_common import state_dict
    sd = state_dict(seed)
    sd["decoder.decoder.fc.bias"] = sd["decoder.decoder.fc.bias"].clone()
    sd["decoder.decoder.fc.bias"][eos] += eos_bias
    return sd


def topk_lower_index(v: torch.Tensor, k: int):
    """(values, indices) of the k best along the last dimension: higher value first, then lower index; NaN counts as -inf"""
    key = torch.where(torch.isnan(v), torch.full_like(v, NINF), v)
    order = torch.sort(key, dim=-1, descending=True, stable=True).indices[..., :k]
    return torch.gather(key, -1, order), order


def beam_step_ref(logits: torch.Tensor, seq: torch.Tensor, N: int, B: int, C: int, eos: int):
    """steps 2-4 and 7 of one time step -> {score, sym, pred, seq (masked), cand (N, B C): every candidate, NaN as -inf}"""
    cand = seq.reshape(N * B, 1) + torch.log_softmax(logits.reshape(N * B, C), dim=1)
    cand = cand.reshape(N, B * C)
    score, f = topk_lower_index(cand, B)
    sym = (f % C).reshape(-1)
    pred = (torch.div(f, C, rounding_mode="floor") + torch.arange(N).reshape(N, 1) * B).reshape(-1)
    score = score.reshape(-1)
    nxt = torch.where(sym == eos, torch.full_like(score, NINF), score)
    return {"score": score, "sym": sym, "pred": pred, "seq": nxt, "cand": torch.where(torch.isnan(cand), torch.full_like(cand, NINF), cand)}


def backtrack_ref(score_hist: torch.Tensor, sym_hist: torch.Tensor, pred_hist: torch.Tensor, N: int, B: int, L: int, eos: int):
    """the walk over [L][R] histories -> {ids (N, L) int64, best_score (N), best_len (N) int64, found (N): eos rows met, final (N, B):
    the slot scores after the walk, sorted}"""
    ids = torch.zeros(N, L, dtype=torch.int64)
    best_score = torch.zeros(N, dtype=score_hist.dtype)
    best_len = torch.zeros(N, dtype=torch.int64)
    found_all = torch.zeros(N, dtype=torch.int64)
    final = torch.zeros(N, B, dtype=score_hist.dtype)
    for n in range(N):
        rows = slice(n * B, n * B + B)
        s, order = topk_lower_index(score_hist[L - 1, rows], B)
        s = score_hist[L - 1, rows][order].clone()
        ptr = (order + n * B).tolist()
        length = [L] * B
        syms = [[0] * L for _ in range(B)]
        found = 0
        for t in range(L - 1, -1, -1):
            for k in range(B):
                syms[k][t] = int(sym_hist[t, ptr[k]])
                ptr[k] = int(pred_hist[t, ptr[k]])
            for b in range(B - 1, -1, -1):
                r = n * B + b
                if int(sym_hist[t, r]) == eos:
                    k = B - 1 - (found % B)
                    found += 1
                    ptr[k], syms[k][t], s[k], length[k] = int(pred_hist[t, r]), eos, score_hist[t, r], t + 1
        fs, order = topk_lower_index(s, B)
        k = int(order[0])
        ids[n] = torch.tensor(syms[k])
        best_score[n], best_len[n], found_all[n], final[n] = s[k], length[k], found, fs
    return {"ids": ids, "best_score": best_score, "best_len": best_len, "found": found_all, "final": final}


def top_gaps(cand: torch.Tensor, B: int) -> torch.Tensor:
    """(N,) the smallest gap between adjacent ranks among the best B + 1 FINITE candidates of every image (inf where fewer than two)"""
    v, _ = topk_lower_index(cand, min(B + 1, cand.shape[1]))
    d = v[:, :-1] - v[:, 1:]
    d = torch.where(torch.isfinite(v[:, 1:]) & torch.isfinite(v[:, :-1]), d, torch.full_like(d, float("inf")))
    return d.min(dim=1).values if d.shape[1] else torch.full((cand.shape[0],), float("inf"), dtype=cand.dtype)


def beam_search_ref(p, feats: torch.Tensor, C: int, L: int, B: int, eos: int, dtype=torch.float64, prefix="decoder.decoder"):
    """the whole decode on encoder features (N, T, D) with the weights `p` (state_dict of the recogniser), in `dtype` -> histories
    score / sym / pred [L][R], gaps [L][N] (top_gaps of every step), and everything backtrack_ref returns"""
    from oracle import aster_oracle as A
    q = {k: v.to(dtype) for k, v in p.items() if k.startswith(prefix) and v.is_floating_point()}
    N = feats.shape[0]
    R = N * B
    x = feats.to(dtype).repeat_interleave(B, dim=0)
    a = prefix + ".attention_unit"
    xproj = torch.nn.functional.linear(x, q[a + ".xEmbed.weight"], q[a + ".xEmbed.bias"])
    s = x.new_zeros(R, q[prefix + ".gru.weight_hh_l0"].shape[1])
    seq = x.new_full((N, B), NINF)
    seq[:, 0] = 0.0
    seq = seq.reshape(-1)
    y = torch.full((R,), C, dtype=torch.long)
    hist = {"score": [], "sym": [], "pred": [], "gaps": []}
    for _ in range(L):
        logits, s_new = A.decoder_step(q, prefix, x, xproj, s, y)
        st = beam_step_ref(logits, seq, N, B, C, eos)
        s, seq, y = s_new[st["pred"]], st["seq"], st["sym"]
        for k in ("score", "sym", "pred"):
            hist[k].append(st[k])
        hist["gaps"].append(top_gaps(st["cand"], B))
    out = {k: torch.stack(v) for k, v in hist.items()}
    out.update(backtrack_ref(out["score"], out["sym"], out["pred"], N, B, L, eos))
    return out


def conditions(score, sym, pred, gaps, N: int, B: int, L: int, eos: int):
    """the fixture's conditions from stored histories -> dict of booleans / figures (see make_golden_aster_beam.py)"""
    score, sym, pred, gaps = (torch.as_tensor(np.asarray(v)) for v in (score, sym, pred, gaps))
    bt = backtrack_ref(score.double(), sym.long(), pred.long(), N, B, L, eos)
    ended = (sym.long() == eos).reshape(L, N, B)
    final_gap = (bt["final"][:, 0] - bt["final"][:, 1]).min().item() if B > 1 else float("inf")
    return {
        "finite": bool(torch.isfinite(score).all()),
        "min_gap": float(gaps.min()),
        "final_gap": float(final_gap),
        "never_eos": [bool(not ended[:, n].any()) for n in range(N)],                                  # (a)
        "ends_early": [bool(bt["best_len"][n] < L and bt["ids"][n, bt["best_len"][n] - 1] == eos) for n in range(N)],   # (b)
        "wraps": [bool(bt["found"][n] > B) for n in range(N)],                                          # (c)
        "together": [bool((ended[:, n].sum(1) >= 2).any()) for n in range(N)],                          # (d)
        "bt": bt,
    }


def conditions_hold(c) -> bool:
    return (c["finite"] and c["min_gap"] >= GAP and c["final_gap"] >= GAP and any(c["never_eos"]) and any(c["ends_early"])
            and any(c["wraps"]) and any(c["together"]))
