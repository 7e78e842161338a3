"""GPU: the ASTER beam-search decode (csrc/aster.hip: tpgsr_aster_attention_rows, tpgsr_beam_step, tpgsr_gather_rows, tpgsr_beam_backtrack;
AttentionRecognitionHead.beam_search; RecognizerBuilder(beam_width=k)) against the fixture generated from the imported reference
(tests/golden/aster_beam.npz) and against the float64 restatement of tests/aster_beam_common.py.

Bounds.  Decisions (symbols, predecessors, ids, lengths) are exact: the fixture keeps the best B + 1 candidates of every step GAP = 1e-3
apart, the synthetic cases check the same gap on their own float64 candidates, and exact ties are planted on purpose (they go to the lower
index).  Scores of the whole decode: within GAP / 8 = 1.25e-4 of float64 (a decision flips only if two scores together move by GAP).
Scores of tpgsr_beam_step alone: the `arith` rule of tests/kernel_table.py, e_gpu <= 4 e_ref32 + 4 * 2^-24 with e = max |got - ref64| /
max |ref64| over the finite entries; the non-finite entries are -inf in both.  Copies (gather, the backtrack's scores) are bitwise.

Observed on an MI355X: step scores of the whole decode within 9.4e-6 of float64 (bound 1.25e-4); tpgsr_beam_step e_gpu <= 1.1e-7,
0.04 - 0.23 of its bound; DESIGN.md section 8, row "ASTER beam search"."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import aster_oracle as A  # noqa: E402
from tests import aster_common  # noqa: E402
from tests.aster_beam_common import (GAP, SCORE_TOL, backtrack_ref, beam_search_ref, beam_state_dict, beam_step_ref, fixture,  # noqa: E402
                                     top_gaps)
from kernel_table import FLOOR, _gen, err  # noqa: E402

DEV = "cuda"
NINF = float("-inf")
GUARD = 16


def K():
    from tpgsr_amd import kernels
    return kernels


def _builder(max_len, beam_width):
    from tpgsr_amd.model import recognizer
    voc = A.get_vocabulary("all")
    return recognizer.RecognizerBuilder(arch="ResNet_ASTER", rec_num_classes=len(voc), sDim=512, attDim=512, max_len_labels=max_len,
                                        eos=voc.index("EOS"), STN_ON=True, beam_width=beam_width), voc


@pytest.fixture(scope="module")
def g():
    return fixture()


@pytest.fixture(scope="module")
def beam_sd(g):
    return beam_state_dict(int(g["seed"]), int(g["eos"]), float(g["eos_bias"]))


@pytest.fixture(scope="module")
def beam_net(g, beam_sd):
    """the recogniser with the beam fixture's weights, beam_width = 5"""
    net, _ = _builder(int(g["max_len"]), 5)
    net.load_state_dict(beam_sd, strict=True)
    return net.to(DEV).eval()


@pytest.fixture(scope="module")
def greedy_net():
    """the recogniser with the greedy fixture's weights (tests/golden/aster_eval.npz), beam_width = 0"""
    e = aster_common.fixture()
    net, _ = _builder(int(e["max_len"]), 0)
    net.load_state_dict(aster_common.state_dict(int(e["seed"])), strict=True)
    return net.to(DEV).eval()


# ---- 1. the reference fixture ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [5, 3])
def test_beam_search_matches_the_reference_fixture(g, beam_net, B):
    eos = int(g["eos"])
    feats = torch.tensor(g["feats"]).to(DEV)
    ids, ones = beam_net.decoder.beam_search(feats, B, eos)
    d = beam_net.decoder.beam_decode(feats, B, eos)
    torch.cuda.synchronize()
    assert ids.dtype == torch.int64 and ones.dtype == torch.int64 and bool((ones == 1).all()) and ones.shape == ids.shape
    want = torch.tensor(g[f"ids_b{B}"])
    dev_score = (d["score"].cpu().double() - torch.tensor(g[f"score_hist_b{B}"])).abs().max().item()
    dev_best = (d["best_score"].cpu().double() - torch.tensor(g[f"best_score_b{B}"])).abs().max().item()
    print(f"B={B}: max |step score - float64| {dev_score:.3e}, max |best score - float64| {dev_best:.3e} (bound {SCORE_TOL:.3e})")
    assert torch.equal(ids.cpu(), want), (ids.tolist(), want.tolist())
    assert torch.equal(d["ids"].cpu(), want)
    assert torch.equal(d["best_len"].cpu().long(), torch.tensor(g[f"best_len_b{B}"]))
    assert torch.equal(d["sym"].cpu(), torch.tensor(g[f"sym_hist_b{B}"])) and torch.equal(d["pred"].cpu(), torch.tensor(g[f"pred_hist_b{B}"]))
    assert bool(torch.isfinite(d["score"]).all())
    assert dev_score <= SCORE_TOL and dev_best <= SCORE_TOL


# ---- 2. tpgsr_beam_step alone ---------------------------------------------------------------------------------------------------------
def _step_inputs(N, B, C, kind):
    """float32 logits [R][C] and running scores [R]; the random kinds keep the float64 candidates' best B + 1 at least GAP apart"""
    R = N * B
    for s in range(64):
        gen = _gen("beam-step", N, B, C, kind, s)
        logits = torch.randn(R, C, generator=gen) * 3
        seq = -torch.rand(R, generator=gen) * 4
        if kind == "first-step":                               # the decode's own start: beam 0 alive, the others -inf
            seq = torch.full((N, B), NINF)
            seq[:, 0] = 0.0
            seq = seq.reshape(-1)
        if kind == "some-dead" and B > 1:
            seq[torch.arange(R) % B == B - 1] = NINF           # the last beam of every image ended in the step before
        if kind == "dead-image":
            seq[:B] = NINF                                     # every beam of image 0 ended: all of its candidates are -inf
        if kind == "nan-row":
            logits[R - 1] = float("nan")                       # log_softmax of a row with a NaN is NaN throughout: counts as -inf
            logits[0, C // 2] = float("nan")
        cand = beam_step_ref(logits.double(), seq.double(), N, B, C, -1)["cand"]
        if float(top_gaps(cand, B).min()) >= GAP:
            return logits, seq
    raise AssertionError("no generator keeps the gap")


def _run_step(logits, seq, N, B, C, eos):
    R = N * B
    buf = {"score": torch.full((R + 2 * GUARD,), -7.0, device=DEV), "sym": torch.full((R + 2 * GUARD,), -7, dtype=torch.int32, device=DEV),
           "pred": torch.full((R + 2 * GUARD,), -7, dtype=torch.int32, device=DEV), "seq": torch.full((R + 2 * GUARD,), -7.0, device=DEV)}
    buf["seq"][GUARD:GUARD + R] = seq.to(DEV)
    K().beam_step(logits.to(DEV).contiguous(), buf["seq"][GUARD:GUARD + R], N, B, C, eos, buf["score"][GUARD:GUARD + R],
                  buf["sym"][GUARD:GUARD + R], buf["pred"][GUARD:GUARD + R])
    torch.cuda.synchronize()
    out = {}
    for k, v in buf.items():
        v = v.cpu()
        assert bool((v[:GUARD] == -7).all()) and bool((v[GUARD + R:] == -7).all()), f"guard words around {k} were written"
        out[k] = v[GUARD:GUARD + R]
    return out


def _check_step(logits, seq, N, B, C, eos, tag):
    got = _run_step(logits, seq, N, B, C, eos)
    r64 = beam_step_ref(logits.double(), seq.double(), N, B, C, eos)
    r32 = beam_step_ref(logits, seq, N, B, C, eos)
    rows = torch.arange(N * B) // B
    assert bool(((got["sym"] >= 0) & (got["sym"] < C)).all()), (tag, got["sym"].tolist())                       # the range guarantee
    assert bool(((got["pred"] >= rows * B) & (got["pred"] < rows * B + B)).all()), (tag, got["pred"].tolist())
    assert torch.equal(got["sym"].long(), r64["sym"]), (tag, got["sym"].tolist(), r64["sym"].tolist())
    assert torch.equal(got["pred"].long(), r64["pred"]), (tag, got["pred"].tolist(), r64["pred"].tolist())
    for key in ("score", "seq"):
        fin = torch.isfinite(r64[key])
        assert torch.equal(torch.isfinite(got[key]), fin) and bool((got[key][~fin] == NINF).all()), (tag, key)
        if fin.any():
            e_gpu, e32 = err(got[key][fin], r64[key][fin]), err(r32[key][fin], r64[key][fin])
            print(f"{tag} {key}: e_gpu {e_gpu:.2e}  e_ref32 {e32:.2e}  bound {4 * e32 + FLOOR:.2e}")
            assert e_gpu <= 4 * e32 + FLOOR, (tag, key, e_gpu, e32)
    assert torch.equal(torch.isinf(got["seq"]) & torch.isfinite(got["score"]), (r64["sym"] == eos) & torch.isfinite(r64["score"]))


@pytest.mark.parametrize("N,B,C", [(3, 5, 97), (2, 1, 97), (2, 8, 37), (1, 3, 2)])
@pytest.mark.parametrize("kind", ["first-step", "random", "some-dead"])
def test_beam_step_against_float64(N, B, C, kind):
    logits, seq = _step_inputs(N, B, C, kind)
    r = beam_step_ref(logits.double(), seq.double(), N, B, C, -1)
    eos = int(r["sym"][0])                                     # the best candidate of image 0 is an eos: its running score is masked
    _check_step(logits, seq, N, B, C, eos, f"N{N}-B{B}-C{C}-{kind}")


@pytest.mark.parametrize("kind", ["dead-image", "nan-row"])
def test_beam_step_without_finite_candidates(kind):
    N, B, C = 3, 5, 97
    logits, seq = _step_inputs(N, B, C, kind)
    _check_step(logits, seq, N, B, C, 94, kind)


def test_beam_step_all_nan_and_all_dead_stay_in_range():
    """no finite candidate anywhere (NaN logits; -inf everywhere; C < B with every beam dead): candidates are taken in index order"""
    for N, B, C, fill in [(2, 5, 97, float("nan")), (2, 8, 64, NINF), (2, 3, 2, 0.0), (1, 8, 1, 0.0)]:
        logits = torch.full((N * B, C), fill)
        seq = torch.full((N * B,), NINF if fill == 0.0 else 0.0)
        got = _run_step(logits, seq, N, B, C, 1)
        f = torch.arange(B).repeat(N)                          # j-th best = flat candidate j
        base = (torch.arange(N * B) // B) * B
        assert torch.equal(got["sym"].long(), f % C) and torch.equal(got["pred"].long(), base + f // C), (N, B, C, got)
        assert bool((got["score"] == NINF).all()) and bool((got["seq"] == NINF).all())


def test_beam_step_planted_ties_go_to_the_lower_index():
    """equal candidates across beams (identical rows, equal running scores), within a row (c, c + 1; c, c + 64: one lane's strided scan
    against another's), and both at once: exact in float32 and in float64, so the order is the tie rule alone"""
    N, B, C = 2, 5, 97
    row = -1.0 - (torch.arange(C) % 5).float()                 # few distinct values a unit apart: ties everywhere, no near-ties
    logits = row.repeat(N * B, 1)
    logits[:B, 10] = logits[:B, 74] = 2.0                      # image 0: classes 10 and 74 (= 10 + 64) lead in every beam
    logits[B:, 30] = logits[B:, 31] = 2.0                      # image 1: neighbours
    seq = torch.zeros(N * B)
    seq[3] = NINF                                              # image 0: beam 3 is dead
    seq[B + 0] = -0.5                                          # image 1: beam 0 trails, beams 1..4 tie
    got = _run_step(logits, seq, N, B, C, 94)
    assert got["sym"][:B].tolist() == [10, 74, 10, 74, 10] and got["pred"][:B].tolist() == [0, 0, 1, 1, 2]
    assert got["sym"][B:].tolist() == [30, 31, 30, 31, 30] and got["pred"][B:].tolist() == [B + 1, B + 1, B + 2, B + 2, B + 3]
    _check_step(logits, seq, N, B, C, 94, "planted-ties")


# ---- 3. tpgsr_beam_backtrack alone ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 5, 8])
@pytest.mark.parametrize("L", [1, 2, 12])
def test_beam_backtrack_on_random_histories(B, L):
    N, C, eos = 3, 11, 4
    R = N * B
    gen = _gen("beam-backtrack", B, L)
    sym = torch.randint(0, C - 1, (L, R), generator=gen)
    sym = torch.where(sym >= eos, sym + 1, sym)                                                  # no eos yet ...
    sym = torch.where(torch.rand(L, R, generator=gen) < 0.2, torch.full_like(sym, eos), sym)     # ... then about 20 %
    pred = torch.randint(0, B, (L, R), generator=gen) + (torch.arange(R) // B) * B
    score = -(torch.randperm(L * R, generator=gen).float().reshape(L, R) + 1) / 8                # distinct, exactly representable
    score = torch.where(torch.rand(L, R, generator=gen) < 0.1, torch.full_like(score, NINF), score)
    want = backtrack_ref(score.double(), sym, pred, N, B, L, eos)
    ids = torch.full((N * L + 2 * GUARD,), -7, dtype=torch.int32, device=DEV)
    best_score, best_len = torch.full((N + 2,), -7.0, device=DEV), torch.full((N + 2,), -7, dtype=torch.int32, device=DEV)
    K().beam_backtrack(score.to(DEV), sym.int().to(DEV), pred.int().to(DEV), N, B, L, eos, ids[GUARD:GUARD + N * L], best_score[1:N + 1],
                       best_len[1:N + 1])
    torch.cuda.synchronize()
    ids, best_score, best_len = ids.cpu(), best_score.cpu(), best_len.cpu()
    assert bool((ids[:GUARD] == -7).all()) and bool((ids[GUARD + N * L:] == -7).all())
    assert best_score[[0, N + 1]].tolist() == [-7.0, -7.0] and best_len[[0, N + 1]].tolist() == [-7, -7]
    assert torch.equal(ids[GUARD:GUARD + N * L].reshape(N, L).long(), want["ids"]), (ids[GUARD:GUARD + N * L].tolist(), want["ids"].tolist())
    assert torch.equal(best_len[1:N + 1].long(), want["best_len"])
    assert torch.equal(best_score[1:N + 1].double(), want["best_score"])                         # copies: bitwise
    if L == 12 and B <= 3:
        assert bool((want["found"] > B).any())                                                   # the slot index wrapped


# ---- 4. tpgsr_gather_rows -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,W,off", [(7, 13, 0), (40, 512, 0), (5, 8, 1), (300, 4, 0), (1, 1, 0)])
def test_gather_rows_is_exact(R, W, off):
    gen = _gen("gather-rows", R, W)
    src = torch.randn(R * W + off, generator=gen).to(DEV)[off:]                                   # off = 1: 16-byte pieces not allowed
    for name, idx in (("identity", torch.arange(R)), ("reversed", torch.arange(R - 1, -1, -1)), ("random", torch.randint(0, R, (R,), generator=gen)),
                      ("clamped", torch.tensor([-1, R] * R)[:R])):
        dst = torch.full((R * W + 2 * GUARD,), -7.0, device=DEV)
        K().gather_rows(src, idx.int().to(DEV), R, W, dst[GUARD:GUARD + R * W])
        torch.cuda.synchronize()
        want = src.reshape(R, W)[idx.clamp(0, R - 1).to(DEV)]
        assert torch.equal(dst[GUARD:GUARD + R * W].reshape(R, W), want), (name, R, W)
        assert bool((dst[:GUARD] == -7).all()) and bool((dst[GUARD + R * W:] == -7).all()), name


# ---- 5. tpgsr_aster_attention_rows ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,B,T,Ad,D", [(3, 5, 25, 64, 96), (2, 1, 7, 33, 5), (2, 8, 25, 512, 512)])
def test_attention_rows_equals_attention_on_repeated_inputs(N, B, T, Ad, D):
    gen = _gen("attention-rows", N, B, T, Ad, D)
    R = N * B
    xproj, x = torch.randn(N, T, Ad, generator=gen).to(DEV), torch.randn(N, T, D, generator=gen).to(DEV)
    sproj, wv, bv = torch.randn(R, Ad, generator=gen).to(DEV), torch.randn(Ad, generator=gen).to(DEV), torch.randn(1, generator=gen).to(DEV)
    a0, c0 = torch.full((R, T), -7.0, device=DEV), torch.full((R, D), -7.0, device=DEV)
    a1, c1 = torch.full_like(a0, -7.0), torch.full_like(c0, -7.0)
    K().aster_attention(xproj.repeat_interleave(B, 0).contiguous(), sproj, wv, bv, x.repeat_interleave(B, 0).contiguous(), R, T, Ad, D, a0, c0)
    K().aster_attention_rows(xproj, sproj, wv, bv, x, R, B, T, Ad, D, a1, c1)
    torch.cuda.synchronize()
    assert torch.equal(a0, a1) and torch.equal(c0, c1) and bool((a1 != -7).all())
    if B == 1:                                                 # rows_per_seq = 1 IS the existing entry point
        return
    a2, c2 = torch.full_like(a0, -7.0), torch.full_like(c0, -7.0)
    big_xp, big_x = xproj.repeat_interleave(B, 0).contiguous(), x.repeat_interleave(B, 0).contiguous()
    K().aster_attention_rows(big_xp, sproj, wv, bv, big_x, R, 1, T, Ad, D, a2, c2)
    torch.cuda.synchronize()
    assert torch.equal(a0, a2) and torch.equal(c0, c2)


# ---- 6. properties --------------------------------------------------------------------------------------------------------------------
def _up_to_first_eos(row, eos):
    row = row.tolist()
    return row[:row.index(eos) + 1] if eos in row else row


def test_width_one_is_the_greedy_decode(g, greedy_net, beam_net):
    """beam_search(., 1, eos) gives sample()'s ids up to and including the first eos (after it the single beam is dead): on the greedy
    fixture's weights and features, and on the beam fixture's (whose sequences do end)"""
    eos = int(g["eos"])
    e = aster_common.fixture()
    for net, feats in ((greedy_net, torch.tensor(e["feats"])), (beam_net, torch.tensor(g["feats"]))):
        feats = feats.to(DEV)
        greedy, _ = net.decoder.sample([feats, None, None])
        beam, _ = net.decoder.beam_search(feats, 1, eos)
        torch.cuda.synchronize()
        for a, b in zip(greedy.cpu(), beam.cpu()):
            assert _up_to_first_eos(a, eos) == _up_to_first_eos(b, eos), (a.tolist(), b.tolist())
    assert torch.equal(greedy_net.decoder.sample([torch.tensor(e["feats"]).to(DEV), None, None])[0].cpu(), torch.tensor(e["ids"]))


def test_an_image_decoded_alone_gives_its_row_of_the_batch(g, beam_net):
    eos = int(g["eos"])
    feats = torch.tensor(g["feats"]).to(DEV)
    whole = beam_net.decoder.beam_decode(feats, 5, eos)
    for j in range(feats.shape[0]):
        one = beam_net.decoder.beam_decode(feats[j:j + 1].contiguous(), 5, eos)
        torch.cuda.synchronize()
        assert torch.equal(one["ids"][0], whole["ids"][j]) and int(one["best_len"][0]) == int(whole["best_len"][j])
        assert abs(float(one["best_score"][0]) - float(whole["best_score"][j])) <= SCORE_TOL
        assert torch.equal(one["sym"], whole["sym"][:, 5 * j:5 * j + 5])


# ---- 7. the whole recogniser and the evaluator ----------------------------------------------------------------------------------------
def test_recognizer_builder_and_evaluator_with_beam_width_5(g, beam_sd, beam_net):
    """forward == the float64 restatement on the build's OWN encoder features (the rectified image differs from the reference's by 2e-3 in
    fp32, DESIGN.md section 8 row N2: more than GAP, so the end-to-end pin goes through the features); the features keep the margin"""
    from tpgsr_amd.interfaces.super_resolution import TextSREvaluator, parse_aster_data
    eos, C, L = int(g["eos"]), int(g["num_classes"]), int(g["max_len"])
    voc = A.get_vocabulary("all")
    lr = torch.tensor(g["lr"]).to(DEV)
    out = beam_net(parse_aster_data(lr))["output"]
    torch.cuda.synchronize()
    with torch.no_grad():
        want = beam_search_ref(beam_sd, out["encoder_feats"].cpu(), C, L, 5, eos)
    final_gap = float((want["final"][:, 0] - want["final"][:, 1]).min())
    print(f"on the build's features: min step gap {float(want['gaps'].min()):.3e}, final gap {final_gap:.3e}")
    assert bool(torch.isfinite(want["score"]).all()) and float(want["gaps"].min()) >= GAP and final_gap >= GAP
    assert torch.equal(out["pred_rec"].cpu(), want["ids"]), (out["pred_rec"].tolist(), want["ids"].tolist())
    assert out["pred_rec"].dtype == torch.int64 and bool((out["pred_rec_score"] == 1).all()) and out["pred_rec_score"].shape == want["ids"].shape
    strs = TextSREvaluator([], [None], recognizer=beam_net).recognize(lr)
    assert strs == A.get_string_aster(want["ids"], voc), strs


def test_beam_width_0_is_the_greedy_recogniser(greedy_net):
    """the default builder decodes greedily exactly as before: the stored greedy fixture, and sample() on its own features bit for bit"""
    from tpgsr_amd.interfaces.super_resolution import parse_aster_data
    e = aster_common.fixture()
    assert greedy_net.beam_width == 0
    out = greedy_net(parse_aster_data(torch.tensor(e["lr"]).to(DEV)))["output"]
    ids, scores = greedy_net.decoder.sample([out["encoder_feats"], None, None])
    torch.cuda.synchronize()
    assert torch.equal(out["pred_rec"], ids) and torch.equal(out["pred_rec_score"], scores) and scores.dtype == torch.float32
    assert torch.equal(ids.cpu(), torch.tensor(e["ids"]))
    assert (scores.cpu() - torch.tensor(e["scores"])).abs().max().item() < 2e-3


def test_packed_linears_follow_the_weights(g, beam_net):
    """the decode's packed weights are redone when a weight is written in place (its version counter moves) and kept otherwise"""
    dec, eos = beam_net.decoder, int(g["eos"])
    feats = torch.tensor(g["feats"]).to(DEV)
    before = dec._packed_linears()
    assert dec._packed_linears() is before
    with torch.no_grad():
        dec.decoder.fc.weight.neg_()
    assert dec._packed_linears() is not before
    flipped = dec.beam_search(feats, 5, eos)[0].cpu()
    with torch.no_grad():
        dec.decoder.fc.weight.neg_()
    assert not torch.equal(flipped, torch.tensor(g["ids_b5"]))
    assert torch.equal(dec.beam_search(feats, 5, eos)[0].cpu(), torch.tensor(g["ids_b5"]))


# ---- 8. no host synchronisation -------------------------------------------------------------------------------------------------------
def test_beam_decode_does_not_synchronise_the_host(g, beam_net):
    """the whole beam_search call under torch's sync debug mode "error".  The weights are packed by the decode before it (once per set of
    weights: packing uploads descriptor tables from pageable memory, which synchronises); the cache must hold, or the packing raises here"""
    eos = int(g["eos"])
    feats = torch.tensor(g["feats"]).to(DEV)
    scratch = torch.ones(1, device=DEV)
    beam_net.decoder.beam_search(feats, 5, eos)
    packed = beam_net.decoder._packed_linears()
    assert beam_net.decoder._packed_linears() is packed
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            scratch.item()
            honoured = False
        except RuntimeError:
            honoured = True
        if honoured:
            ids, ones = beam_net.decoder.beam_search(feats, 5, eos)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    if not honoured:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') is not honoured by this build: .item() did not raise")
    torch.cuda.synchronize()
    assert torch.equal(ids.cpu(), torch.tensor(g["ids_b5"]))
