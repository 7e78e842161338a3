#!/usr/bin/env python
"""Fixture for the ASTER beam-search decode (AttentionRecognitionHead.beam_search, attention_recognition_head.py:68-184), generated from
the GENUINE reference imported from /root/reference (build container only), like make_golden_aster.py.  Two environment shims around the
call: `Tensor.cuda` = identity (the reference calls .cuda() unconditionally), and `Tensor.__truediv__` of an integer tensor by an integer
= floor division, the torch < 1.5 meaning line 111 was written for.  Stores inputs + expected outputs only; the weights are rebuilt from the
stored recipe seed (tests/aster_beam_common.beam_state_dict).

The generator ASSERTS that the float64 restatement (tests/aster_beam_common.py) gives the reference's ids, and it refuses to write unless
  * every stored score of every step is finite (the case in which torch.topk's order is unspecified does not occur),
  * at every step, for every image and both widths, the best B + 1 finite candidates are pairwise >= GAP = 1e-3 apart, and so are the two
    best final slot scores,
  * among the four images (B = 5): (a) one where no beam ever emits eos, (b) one whose result ends with eos before step L, (c) one where
    more than B eos rows are met in the walk (the slot index wraps), (d) one step where two beams of an image emit eos together,
  * the same margin holds at B = 5 on the features the oracle's encoder makes of the stored images (the whole-recogniser test decodes the
    build's own features, which differ from those by fp32 rounding).

    python tests/golden/make_golden_aster_beam.py        # rewrites tests/golden/aster_beam.npz"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

MAX_LEN, WIDTHS, N_IMG = 12, (5, 3), 4
PIPE_GAP = 2e-3        # margin asked of the oracle's whole-pipeline features: twice GAP, the build's features are not bit-equal to them


def reference_beam_search(head, feats, width, eos):
    """the genuine beam_search under the integer-division shim"""
    true_div = torch.Tensor.__truediv__

    def div(self, other):
        if not self.is_floating_point() and isinstance(other, int):
            return torch.div(self, other, rounding_mode="floor")
        return true_div(self, other)

    torch.Tensor.__truediv__ = div
    try:
        with torch.no_grad():
            ids, ones = head.beam_search(feats, width, eos)
    finally:
        torch.Tensor.__truediv__ = true_div
    assert torch.equal(ones, torch.ones_like(ids))
    return ids


def pipeline_feats(sd, lr):
    from oracle import aster_oracle as A
    images = A.parse_aster_data(lr)
    stn_in = torch.nn.functional.interpolate(images, A.TPS_INPUT, mode="bilinear", align_corners=True)
    _, ctrl = A.stn_head(sd, "stn_head", stn_in)
    rect, _ = A.O.tps_transform(sd, "tps", images, ctrl, A.TPS_OUTPUT)
    return A.encoder(sd, "encoder", rect)


def main():
    for name in ("IPython", "cv2"):
        m = types.ModuleType(name)
        m.embed = lambda *a, **k: None
        sys.modules.setdefault(name, m)
    tv = types.ModuleType("torchvision")
    for sub in ("models", "transforms", "datasets"):
        m = types.ModuleType("torchvision." + sub)
        setattr(tv, sub, m)
        sys.modules["torchvision." + sub] = m
    sys.modules.setdefault("torchvision", tv)
    torch.Tensor.cuda = lambda self, *a, **k: self
    sys.path.insert(0, "/root/reference")
    import warnings
    warnings.filterwarnings("ignore")
    from model.recognizer.attention_recognition_head import AttentionRecognitionHead
    from oracle import aster_oracle as A
    import aster_beam_common as BC

    voc = A.get_vocabulary("all")
    C, eos = len(voc), voc.index("EOS")
    assert (C, eos) == (97, 94)
    head = AttentionRecognitionHead(num_classes=C, in_planes=512, sDim=512, attDim=512, max_len_labels=MAX_LEN).eval()
    lr = torch.rand(N_IMG, 4, 16, 64, generator=torch.Generator().manual_seed(32))
    for k in range(200):
        seed, eos_bias = 5000 + k, 4.0 + 0.05 * k
        sd = BC.beam_state_dict(seed, eos, eos_bias)
        feats = torch.randn(N_IMG, 25, 512, generator=torch.Generator().manual_seed(seed))
        with torch.no_grad():
            runs = {B: BC.beam_search_ref(sd, feats, C, MAX_LEN, B, eos) for B in WIDTHS}
            conds = {B: BC.conditions(r["score"], r["sym"], r["pred"], r["gaps"], N_IMG, B, MAX_LEN, eos) for B, r in runs.items()}
        c5 = conds[WIDTHS[0]]
        print(f"seed {seed}: " + "; ".join(f"B={B} finite {c['finite']} gap {c['min_gap']:.2e} final {c['final_gap']:.2e}" for B, c in conds.items())
              + f"; (a) {c5['never_eos']} (b) {c5['ends_early']} (c) {c5['wraps']} (d) {c5['together']}", flush=True)
        if not (BC.conditions_hold(c5) and all(c["finite"] and min(c["min_gap"], c["final_gap"]) >= BC.GAP for c in conds.values())):
            continue
        with torch.no_grad():
            pf = pipeline_feats(sd, lr)
            pr = BC.beam_search_ref(sd, pf, C, MAX_LEN, WIDTHS[0], eos)
        pc = BC.conditions(pr["score"], pr["sym"], pr["pred"], pr["gaps"], N_IMG, WIDTHS[0], MAX_LEN, eos)
        print(f"   whole pipeline: finite {pc['finite']} gap {pc['min_gap']:.2e} final {pc['final_gap']:.2e}", flush=True)
        if pc["finite"] and min(pc["min_gap"], pc["final_gap"]) >= PIPE_GAP:
            break
    else:
        raise SystemExit("no seed meets the fixture's conditions")

    head.load_state_dict({k[len("decoder."):]: v for k, v in sd.items() if k.startswith("decoder.")}, strict=True)
    store = {"lr": lr.numpy(), "feats": feats.numpy(), "seed": np.array(seed), "eos_bias": np.array(eos_bias), "eos": np.array(eos),
             "max_len": np.array(MAX_LEN), "num_classes": np.array(C), "widths": np.array(WIDTHS), "gap": np.array(BC.GAP),
             "pipe_ids_b5": pr["ids"].numpy(), "pipe_min_gap": np.array(min(pc["min_gap"], pc["final_gap"]))}
    for B in WIDTHS:
        ref_ids = reference_beam_search(head, feats, B, eos)
        r = runs[B]
        assert torch.equal(r["ids"], ref_ids), (B, r["ids"].tolist(), ref_ids.tolist())        # restatement == reference, before writing
        print(f"B={B}: reference ids == float64 restatement ids; strings {A.get_string_aster(ref_ids, voc)}; lengths {r['best_len'].tolist()}")
        store.update({f"ids_b{B}": ref_ids.numpy(), f"score_hist_b{B}": r["score"].numpy(), f"sym_hist_b{B}": r["sym"].numpy().astype(np.int32),
                      f"pred_hist_b{B}": r["pred"].numpy().astype(np.int32), f"gaps_b{B}": r["gaps"].numpy(),
                      f"best_score_b{B}": r["best_score"].numpy(), f"best_len_b{B}": r["best_len"].numpy()})
    np.savez_compressed(os.path.join(HERE, "aster_beam.npz"), **store)
    print("wrote aster_beam.npz; seed", seed, "eos bias", eos_bias)


if __name__ == "__main__":
    main()
