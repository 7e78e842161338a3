"""GPU: engine.TConvStrip and engine.FoldedDgrad, one layer at a time through the harness of tests/engine_layer_common.py (the engine's own layer
objects, eagerly), against stock PyTorch in float64 on the CPU, element by element.

TConvStrip -- InfoGen's ConvTranspose2d on the H = 1 text strip (model/tsrn.py:81-108) as a 1x3 convolution over the zero-dilated strip: pack
kind 4 with the 37 classes padded to 40 channels (`cin_ld` / `d_ld`), forward, the strided data gradient and the weight gradient with its
padded slab rows skipped by the reduce.  Weights [37][64][3][3] at stride 2, padding 1 on a 26-column strip (tconv1's geometry) and
[64][32][3][3] at stride 1, padding 0 on 7 columns (tconv4's), N = 2.  y, dx and dW against F.conv_transpose2d and its autograd; the weight
gradient in the arena has exactly the parameter's shape (rows kh != 1 get no gradient on an H = 1 strip, in the reference too).
FoldedDgrad -- the data gradient of block1's 9x9 convolution with few input channels (model/tsrn.py:28) folded into a 9x1 convolution with the
kw taps in the columns (pack kind 7) + tpgsr_shiftsum_nhwc: weights [64][4][9][9] and [64][3][9][9] (KS Ci not a multiple of 4), maps 1x16x64
and 2x5x7, against the input gradient of F.conv2d(x, w, padding=4).

Policies and bounds as tests/test_engine_gru_layer_gpu.py: x3 and f32 5e-6 (values, data gradients) / 1e-5 (weight gradient), x2 2e-5, bf16 2e-2;
e = max |got - ref64| / max |ref64|.  Every test asserts the launch list it produced.

OBSERVED on an MI355X, worst e / bound per policy (`test_zz_report` prints it), all tests passing:
  TConvStrip   x3 0.03   x2 0.31   bf16 0.14   f32 0.14
  FoldedDgrad  x3 0.04   x2 0.21   bf16 0.11   f32 0.10
"""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import engine_layer_common as E  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
STRIPS, FOLDS = E.strip_cases(), E.fold_cases()
WORST = {}


def _compare(case, got, ref, policy, param_keys=()):
    lim = E.limits(policy)
    bad = []
    assert set(got) == set(ref)
    for key in sorted(ref):
        assert tuple(got[key].shape) == tuple(ref[key].shape), (key, tuple(got[key].shape), tuple(ref[key].shape))
        bound = lim[1] if key in param_keys else lim[0]
        e = E.err(got[key], ref[key])
        tag = f"{type(case).__name__} {policy}"
        WORST[tag] = max(WORST.get(tag, 0.0), e / bound)
        print(f"{case.id} {policy} {key}: e {e:.2e}  bound {bound:.0e}  ratio {e / bound:.2f}")
        if not e <= bound:
            bad.append(f"{key}: e {e:.3e} > {bound:.0e}")
    assert not bad, f"{case.id} {policy}: " + "; ".join(bad)


@pytest.mark.parametrize("policy", E.POLICIES)
@pytest.mark.parametrize("case", STRIPS, ids=[c.id for c in STRIPS])
def test_tconv_strip_vs_fp64(case, policy):
    with E.conv_prec(policy):
        got, names = E.run_strip(case, DEV)
    assert names == case.expected_launches(policy), names
    _compare(case, got, case.reference(), policy, param_keys=("dw",))


@pytest.mark.parametrize("policy", E.POLICIES)
@pytest.mark.parametrize("case", FOLDS, ids=[c.id for c in FOLDS])
def test_folded_dgrad_vs_fp64(case, policy):
    with E.conv_prec(policy):
        got, names = E.run_fold(case, DEV)
    assert names == case.expected_launches(policy), names
    _compare(case, got, case.reference(), policy)


def test_zz_report():
    for tag in sorted(WORST):
        print(f"engine {tag}: worst e / bound {WORST[tag]:.2f}")
