"""Attention GRU decoder (reference: model/recognizer/attention_recognition_head.py): AttentionUnit (:168-218), DecoderUnit (:221-268),
AttentionRecognitionHead.sample (:47-67) = the greedy decode, .beam_search (:68-184) = the decode the reference's evaluator uses.  Same
state_dict layout.  The reference's beam_search divides an integer tensor with `/` (:111), floor division before torch 1.5; it is pinned
here against the reference run with that meaning restored (tests/golden/make_golden_aster_beam.py).  torch.topk's order among equal
values is unspecified; here equal candidates go to the lower index."""
import torch
from torch import nn

from ... import functional as Fh
from ... import kernels as K
from ..nn_params import LinearParams, _NoForward, _uniform

MAX_BEAM_WIDTH = 8               # tpgsr_beam_step (include/tpgsr_hip.h): 1 <= B <= 8 and B * C <= 512 candidates per image
MAX_BEAM_CANDIDATES = 512


class AttentionUnit(nn.Module):
    def __init__(self, sDim, xDim, attDim):
        super().__init__()
        self.sDim, self.xDim, self.attDim = sDim, xDim, attDim
        self.sEmbed = LinearParams(sDim, attDim)
        self.xEmbed = LinearParams(xDim, attDim)
        self.wEmbed = LinearParams(attDim, 1)


class _EmbeddingParams(_NoForward):
    def __init__(self, num, dim):
        super().__init__()
        self.num_embeddings, self.embedding_dim = num, dim
        self.weight = nn.Parameter(torch.randn(num, dim))


class _GRUCellParams(_NoForward):
    """nn.GRU(input_size, hidden_size, batch_first=True), one layer, one direction"""

    def __init__(self, input_size, hidden_size):
        super().__init__()
        self.input_size, self.hidden_size = input_size, hidden_size
        b = 1.0 / hidden_size ** 0.5
        self.weight_ih_l0 = nn.Parameter(_uniform(torch.empty(3 * hidden_size, input_size), b))
        self.weight_hh_l0 = nn.Parameter(_uniform(torch.empty(3 * hidden_size, hidden_size), b))
        self.bias_ih_l0 = nn.Parameter(_uniform(torch.empty(3 * hidden_size), b))
        self.bias_hh_l0 = nn.Parameter(_uniform(torch.empty(3 * hidden_size), b))

    def flatten_parameters(self):
        pass


class DecoderUnit(nn.Module):
    def __init__(self, sDim, xDim, yDim, attDim):
        super().__init__()
        self.sDim, self.xDim, self.yDim, self.attDim, self.emdDim = sDim, xDim, yDim, attDim, attDim
        self.attention_unit = AttentionUnit(sDim, xDim, attDim)
        self.tgt_embedding = _EmbeddingParams(yDim + 1, self.emdDim)        # the last row is <BOS>
        self.gru = _GRUCellParams(xDim + self.emdDim, sDim)
        self.fc = LinearParams(sDim, yDim)


class AttentionRecognitionHead(nn.Module):
    """input: encoder features (N, T, in_planes); sample(): greedy ids (N, max_len_labels) int64 and their softmax scores;
    beam_search(): the best hypothesis' ids (N, max_len_labels) int64 and ones"""

    def __init__(self, num_classes, in_planes, sDim, attDim, max_len_labels):
        super().__init__()
        self.num_classes, self.in_planes, self.sDim, self.attDim, self.max_len_labels = num_classes, in_planes, sDim, attDim, max_len_labels
        self.decoder = DecoderUnit(sDim=sDim, xDim=in_planes, yDim=num_classes, attDim=attDim)

    def forward(self, x):
        raise RuntimeError("teacher-forced decoding (training) is not part of the evaluation path; use sample()")

    def beam_search(self, x, beam_width, eos):
        """(N, T, in_planes) features -> (ids (N, max_len_labels) int64, ones_like(ids)): the best of `beam_width` hypotheses per image, as
        the reference's beam_search computes it.  beam_width in 1..8, eos an integer class id (ValueError otherwise, before any launch)."""
        ids = self.beam_decode(x, beam_width, eos)["ids"]
        return ids, torch.ones_like(ids)

    def _packed_linears(self):
        """the five linears of a decoder step, packed once per set of weights: packing uploads a descriptor table per operand, a pageable
        host-to-device copy that synchronises, so the first decode after the weights (or the arithmetic policy) change pays for it and the
        following ones make no synchronising call at all.  Keyed on the parameters' storage and version counters."""
        d, au = self.decoder, self.decoder.attention_unit
        params = (au.xEmbed.weight, au.xEmbed.bias, au.sEmbed.weight, au.sEmbed.bias, d.gru.weight_ih_l0, d.gru.bias_ih_l0,
                  d.gru.weight_hh_l0, d.gru.bias_hh_l0, d.fc.weight, d.fc.bias)
        key = (K.POLICY, K.CONV_TERMS) + tuple((p.data_ptr(), p._version) for p in params)
        if getattr(self, "_packed", (None, None))[0] != key:
            self._packed = (key, tuple(Fh.PackedLinear(params[i], params[i + 1]) for i in range(0, 10, 2)))
        return self._packed[1]

    def beam_decode(self, x, beam_width, eos):
        """the decode behind beam_search, with what the reference computes and drops: {ids (N, L) int64, best_score (N), best_len (N) int32,
        score / sym / pred: the [L][R] histories}.  R = N * beam_width decoder rows, row n * beam_width + b, all beams of an image on one
        copy of its features; per step the beam_width best of beam_width * num_classes candidates per image; one backtrack over the stored
        histories at the end.  Equal candidates go to the lower index.  Nothing is read back from the device: the loop's control flow
        depends on no device value."""
        if isinstance(beam_width, bool) or not isinstance(beam_width, int) or not 1 <= beam_width <= MAX_BEAM_WIDTH:
            raise ValueError(f"beam_search: beam_width must be an integer in 1..{MAX_BEAM_WIDTH} (got {beam_width!r})")
        if isinstance(eos, bool) or not isinstance(eos, int):
            raise ValueError(f"beam_search: eos must be the integer class id of the end-of-sequence symbol (got {eos!r})")
        C, B, L = self.num_classes, beam_width, self.max_len_labels
        if B * C > MAX_BEAM_CANDIDATES:
            raise ValueError(f"beam_search: beam_width * num_classes = {B * C} candidates per image, the kernel holds {MAX_BEAM_CANDIDATES}")
        feats = x[0] if isinstance(x, (list, tuple)) else x
        if feats.requires_grad:
            raise RuntimeError("AttentionRecognitionHead.beam_search is an evaluation path (no gradient)")
        with torch.no_grad():
            d, au = self.decoder, self.decoder.attention_unit
            N, T, D = feats.shape
            R = N * B
            dev = feats.device
            feats = feats.contiguous()
            xe, se, gi_l, gh_l, fc = self._packed_linears()
            xproj = xe(feats.reshape(N * T, D))                                   # per image: the beams of an image share it (and feats)
            s = torch.zeros(R, self.sDim, device=dev)
            s2 = torch.empty_like(s)
            seq = torch.full((N, B), float("-inf"), device=dev)                   # running scores: beam 0 of every image starts alive
            seq[:, 0] = 0.0
            y = torch.full((R,), C, dtype=torch.int32, device=dev)                # <BOS>
            score_hist = torch.empty(L, R, device=dev)
            sym_hist = torch.empty(L, R, dtype=torch.int32, device=dev)
            pred_hist = torch.empty(L, R, dtype=torch.int32, device=dev)
            alpha, ctx = torch.empty(R, T, device=dev), torch.empty(R, D, device=dev)
            inp = torch.empty(R, self.attDim + D, device=dev)
            sproj, logits = torch.empty(R, self.attDim, device=dev), torch.empty(R, C, device=dev)
            gi, gh = torch.empty(R, 3 * self.sDim, device=dev), torch.empty(R, 3 * self.sDim, device=dev)
            wv, bv, emb = au.wEmbed.weight.reshape(-1).contiguous(), au.wEmbed.bias, d.tgt_embedding.weight
            for i in range(L):
                se(s, out=sproj)
                K.aster_attention_rows(xproj, sproj, wv, bv, feats, R, B, T, self.attDim, D, alpha, ctx)
                K.embed_concat(y, emb, C + 1, self.attDim, ctx, D, R, inp)
                K.gru_cell(gi_l(inp, out=gi), gh_l(s, out=gh), s, R, self.sDim, s2)
                K.beam_step(fc(s2, out=logits), seq, N, B, C, eos, score_hist[i], sym_hist[i], pred_hist[i])
                K.gather_rows(s2, pred_hist[i], R, self.sDim, s)                  # the NEW state, reordered by predecessor
                y = sym_hist[i]
            ids = torch.empty(N, L, dtype=torch.int32, device=dev)
            best_score, best_len = torch.empty(N, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
            K.beam_backtrack(score_hist, sym_hist, pred_hist, N, B, L, eos, ids, best_score, best_len)
            return {"ids": ids.long(), "best_score": best_score, "best_len": best_len, "score": score_hist, "sym": sym_hist,
                    "pred": pred_hist}

    def sample(self, x):
        feats = x[0] if isinstance(x, (list, tuple)) else x
        if feats.requires_grad:
            raise RuntimeError("AttentionRecognitionHead.sample is an evaluation path (no gradient)")
        with torch.no_grad():
            d, au = self.decoder, self.decoder.attention_unit
            N, T, D = feats.shape
            dev = feats.device
            feats = feats.contiguous()
            lin = Fh.PackedLinear
            xe, se, gi_l, gh_l, fc = (lin(au.xEmbed.weight, au.xEmbed.bias), lin(au.sEmbed.weight, au.sEmbed.bias),
                                      lin(d.gru.weight_ih_l0, d.gru.bias_ih_l0), lin(d.gru.weight_hh_l0, d.gru.bias_hh_l0),
                                      lin(d.fc.weight, d.fc.bias))
            xproj = xe(feats.reshape(N * T, D))                                   # does not depend on the step (reference recomputes it)
            s = torch.zeros(N, self.sDim, device=dev)
            s2 = torch.empty_like(s)
            y = torch.full((N,), self.num_classes, dtype=torch.int32, device=dev)  # <BOS>
            L = self.max_len_labels
            ids = torch.zeros(N, L, dtype=torch.int32, device=dev)
            scores = torch.zeros(N, L, device=dev)
            alpha, ctx = torch.empty(N, T, device=dev), torch.empty(N, D, device=dev)
            inp = torch.empty(N, self.attDim + D, device=dev)
            wv, bv, emb = au.wEmbed.weight.reshape(-1).contiguous(), au.wEmbed.bias, d.tgt_embedding.weight
            for i in range(L):
                sproj = se(s)
                K.aster_attention(xproj, sproj, wv, bv, feats, N, T, self.attDim, D, alpha, ctx)
                K.embed_concat(y, emb, self.num_classes + 1, self.attDim, ctx, D, N, inp)
                K.gru_cell(gi_l(inp), gh_l(s), s, N, self.sDim, s2)
                s, s2 = s2, s
                K.softmax_max(fc(s), N, self.num_classes, ids, scores, L, i, y)
            return ids.long(), scores
