"""GPU: the three layer classes of tpgsr_amd/engine_crnn.py -- LstmLayer (BidirectionalLSTM: nn.LSTM(nIn, 256, bidirectional) + Linear, with
its ConvLayer / PaddedLinear embedding), and Conv0Im2col -- one layer at a time against stock PyTorch in float64 on the CPU, element by
element (references: model/crnn/crnn.py:5-26 and :45-46); and the three kernels only these layers call, directly: tpgsr_im2col3x3_c1,
tpgsr_col2im3x3_c1, tpgsr_pad_channels.

Harness and references: tests/engine_crnn_layer_common.py (the engine's own layer objects run, eagerly or recorded into a plan).  Layers:
rnn0 512 -> 256 behind the in_scale / in_shift / ReLU loader (embedding: ConvLayer), rnn1 256 -> 37 (PaddedLinear, Cp = 40); maps (N, T):
2x5, 3x26, 1x33 (T > 31: the counter hand-off forward kernel), 64x2 (the batch limit); policies x3, x2, bf16, f32.
Branches (each test asserts the launch list it produced against LstmCase.expected_launches; where K.lstm_seq_coresident answers no, the
engine records the per-step form everywhere and the tests expect exactly that):
  forward    tpgsr_lstm_seq_fwdg (T <= 31)   tpgsr_lstm_seq_fwd (T = 33, or K.LSTM_GRANULE off)
             per step tpgsr_lstm_rec_gemm + tpgsr_lstm_step_fwd (K.LSTM_SEQ / K.LSTM_SEQ_BWD off)
  backward   tpgsr_lstm_seq_bwd              per step tpgsr_lstm_rec_gemm + tpgsr_lstm_step_bwd
  weight gradients   5 x (tpgsr_conv_wgrad, tpgsr_wgrad_reduce)   eager (and f32 recorded: 5 x tpgsr_conv_wgrad, then one reduce program)
             tpgsr_conv_wgrad_batch + tpgsr_wgrad_reduce_program            recorded, split operands: rnn1 one batch of five; rnn0 a batch of three
             (embedding, two hidden sides) and a SECOND batch of two (the input sides, read through the BatchNorm + ReLU loader: another variant)
Compared with e = max |got - ref64| / max |ref64|, every key: e, out, dx and the ten parameter gradients (BatchNorm test: e, out, ds, twelve).
Bounds: the suite's limits, engine_layer_common.limits -- x3 and f32 5e-6 for values and data gradients, 1e-5 for parameter gradients; x2
2e-5; bf16 2e-2.  Keys listed in MODEL_KEYS get, under x2 / bf16 only, the additive term of `model_terms`: 4 x the error of the float64
reference computed with every split-operand GEMM's operands rounded to two / one bf16 terms -- from the reference alone.  No key needed it:
MODEL_KEYS is empty, every bound below is the suite's limit itself (the terms are printed next to each x2 / bf16 figure: 1.5e-5 .. 3.3e-5
under x2, where the worst e was 1.03e-5).

OBSERVED on an MI355X, worst e / bound per policy (`test_zz_report` prints it), all 77 tests passing:
  LstmLayer, eager               x3 0.06   x2 0.51   bf16 0.28   f32 0.33      (x2: rnn.weight_ih_l0_reverse of rnn0-2x5, e 1.03e-5 of 2e-5)
  recorded (batched wgrads)      x3 0.06   x2 0.51          two forward + backward passes   x3 0.06   x2 0.51
  per-step recurrence            x3 0.06   f32 0.24         counter forward, granules off   x3 0.06
  behind a real BatchNorm        x3 0.07   f32 0.34         Conv0Im2col   x3 0.04   x2 0.34   bf16 0.16   f32 0.04
  tpgsr_col2im3x3_c1 0.16 (of 4 e_ref32 + 4 * 2^-24); tpgsr_im2col3x3_c1, tpgsr_pad_channels and recorded-vs-eager e / out / dx: bit for bit
What these tests found: LstmLayer.bwd, run without deferred slab reduces (eagerly, or recorded with TPGSR_DEFER_REDUCE=0), launched its
weight-gradient GEMMs one after another into the ONE stream-ordered slab scratch and reduced afterwards -- every reduce read the last
launch's slabs.  Before the fix: rnn1-2x5, eager, x3 and f32 alike, rnn.weight_hh_l0 e 9.5, rnn.weight_hh_l0_reverse 7.1, rnn.bias_ih_l0 /
rnn.bias_hh_l0 1.6, rnn.weight_ih_l0 1.5 (bound 1e-5); e, out, dx and the recorded default (deferred reduces, buffers of their own) were right.
Mutants tried through this harness (x3): the two directions' `sgn` swapped in the hidden-side weight-gradient geometry -- rnn.weight_hh_l0 e 1.16
and rnn.weight_hh_l0_reverse 0.81 at rnn1-2x5, 0.45 / 0.33 at rnn0-3x26 (eager and recorded), every other key unchanged; `f_coff` dropped from
the W_ih pack -- out e 1.3, e 0.97, dx 0.68 and every weight gradient of order 1.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import engine_crnn_layer_common as C  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = C.lstm_cases()
BY_ID = {c.id: c for c in CASES}
BN_CASES = C.bn_cases()
CONV0 = C.conv0_cases()
WORST = {}
EAGER = {}            # (case id, policy) -> the eager result, shared with the recorded test

# keys whose bound carries the error-model term under x2 / bf16 (the issue's remedy for keys that are right and exceed the suite's limit at
# these contraction lengths): none unless listed here
MODEL_KEYS = {"x2": (), "bf16": ()}
VALUE_KEYS = ("e", "out", "dx", "ds", "y", "dgray")


def _bound(case, key, policy):
    lim = C.limits(policy)
    b = lim[0] if key in VALUE_KEYS else lim[1]
    if key in MODEL_KEYS.get(policy, ()):
        b += case.model_terms(policy)[key]
    return b


def _compare(case, got, ref, policy, tag, keys, scale=1.0):
    bad = []
    model = case.model_terms(policy) if hasattr(case, "model_terms") else {}
    for key in keys:
        assert tuple(got[key].shape) == tuple(ref[key].shape), (key, tuple(got[key].shape), tuple(ref[key].shape))
        r = ref[key] * scale if (scale != 1.0 and key not in VALUE_KEYS) else ref[key]     # (only the arena accumulates)
        bound = _bound(case, key, policy)
        e = C.err(got[key], r)
        if not e == e:
            e = float("inf")                      # a NaN left in a pre-filled buffer
        WORST[tag] = max(WORST.get(tag, 0.0), e / bound)
        print(f"{case.id} {tag} {key}: e {e:.2e}  bound {bound:.1e}  ratio {e / bound:.2f}" + (f"  model term {model[key]:.1e}" if key in model else ""))
        if not e <= bound:
            bad.append(f"{key}: e {e:.3e} > {bound:.1e}")
    assert not bad, f"{case.id} {tag}: " + "; ".join(bad)


LSTM_ALL = ("e", "out", "dx") + C.LSTM_KEYS


@pytest.mark.parametrize("policy", C.POLICIES)
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_lstm_layer_vs_fp64(case, policy):
    with C.conv_prec(policy):
        got, names, _eng = C.run_lstm(case, DEV)
    assert names == case.expected_launches(policy, per_step=not C.persistent(DEV)), names
    EAGER[(case.id, policy)] = got
    _compare(case, got, case.reference(), policy, "LstmLayer " + policy, LSTM_ALL)


@pytest.mark.parametrize("cid,policy", C.RECORDED)
def test_lstm_layer_recorded_batch(cid, policy):
    """recorded into a plan with deferred slab reduces: tpgsr_conv_wgrad_batch and the reduce program compute the parameter gradients;
    e, out and dx come from the same kernels as in the eager run, and hold the same bits"""
    case = BY_ID[cid]
    with C.conv_prec(policy):
        got, names, _eng = C.run_lstm(case, DEV, mode="recorded")
        want = case.expected_launches(policy, "recorded", per_step=not C.persistent(DEV))
        assert names == want, names
        assert names.count("tpgsr_conv_wgrad_batch") == (2 if case.loader == "relu" else 1) and "tpgsr_conv_wgrad" not in names
        assert names[-1] == "tpgsr_wgrad_reduce_program" and "tpgsr_wgrad_reduce" not in names
        eager = EAGER.get((cid, policy))
        if eager is None:
            eager = C.run_lstm(case, DEV)[0]
    _compare(case, got, case.reference(), policy, "recorded " + policy, LSTM_ALL)
    for key in ("e", "out", "dx"):
        assert torch.equal(got[key], eager[key]), f"{cid} {policy}: {key} differs between the recorded and the eager run"


@pytest.mark.parametrize("cid,policy", C.PER_STEP)
def test_lstm_layer_per_step_branch(cid, policy, monkeypatch):
    """K.LSTM_SEQ / K.LSTM_SEQ_BWD off: one tpgsr_lstm_rec_gemm + tpgsr_lstm_step_{fwd,bwd} per time step, within the persistent branch's bounds"""
    from tpgsr_amd import kernels as K
    monkeypatch.setattr(K, "LSTM_SEQ", False)
    monkeypatch.setattr(K, "LSTM_SEQ_BWD", False)
    case = BY_ID[cid]
    with C.conv_prec(policy):
        got, names, eng = C.run_lstm(case, DEV)
    assert names == case.expected_launches(policy, per_step=True), names
    assert names.count("tpgsr_lstm_rec_gemm") == 2 * (case.T - 1) and names.count("tpgsr_lstm_step_fwd") == names.count("tpgsr_lstm_step_bwd") == case.T
    assert not C.seq_timeouts(eng.layer)                 # no persistent launch, no exchange buffer
    _compare(case, got, case.reference(), policy, "per step " + policy, LSTM_ALL)


@pytest.mark.parametrize("cid,policy", C.GRANULE_OFF)
def test_lstm_layer_counter_forward_with_granules_off(cid, policy, monkeypatch):
    """K.LSTM_GRANULE off: tpgsr_lstm_seq_fwd (the arrival-counter hand-off) at T <= 31 as well"""
    from tpgsr_amd import kernels as K
    monkeypatch.setattr(K, "LSTM_GRANULE", False)
    case = BY_ID[cid]
    with C.conv_prec(policy):
        got, names, _eng = C.run_lstm(case, DEV)
    assert names == case.expected_launches(policy, granule=False, per_step=not C.persistent(DEV)), names
    assert ("tpgsr_lstm_seq_fwd" in names) == C.persistent(DEV)
    _compare(case, got, case.reference(), policy, "counter forward " + policy, LSTM_ALL)


@pytest.mark.parametrize("cid,policy", C.TWO_PASSES)
def test_two_backward_passes_accumulate(cid, policy):
    """forward + backward twice on one gradient arena: every parameter gradient is 2 x the reference (the += of the slab reduces), dx is
    overwritten, the guard and the arena's padding are untouched (run_lstm asserts it)"""
    case = BY_ID[cid]
    with C.conv_prec(policy):
        got, names, _eng = C.run_lstm(case, DEV, passes=2)
    assert names == case.expected_launches(policy, passes=2, per_step=not C.persistent(DEV)), names
    _compare(case, got, case.reference(), policy, "two passes " + policy, LSTM_ALL, scale=2.0)


@pytest.mark.parametrize("policy", C.BN_POLICIES)
@pytest.mark.parametrize("case", BN_CASES, ids=[c.id for c in BN_CASES])
def test_first_bilstm_behind_a_real_batchnorm(case, policy):
    """training-mode BatchNorm2d(512) + ReLU in the loader, its backward sums as the epilogue of the BiLSTM's data gradient (x3) or as the
    statistics launch (f32: fuse_stats returns None); ds and the BatchNorm gradients against float64, nothing masked"""
    with C.conv_prec(policy):
        got, names, fused = C.run_bn_lstm(case, DEV)
    assert fused == (policy == "x3")
    assert ("tpgsr_bn_bwd_reduce" in names) == (not fused)
    assert names == case.expected_launches(policy, per_step=not C.persistent(DEV)), names
    _compare(case, got, case.reference(), policy, "behind BatchNorm " + policy, ("e", "out", "ds") + C.BN_KEYS + C.LSTM_KEYS)


@pytest.mark.parametrize("policy", C.POLICIES)
@pytest.mark.parametrize("case", CONV0, ids=[c.id for c in CONV0])
def test_conv0_im2col_vs_fp64(case, policy):
    with C.conv_prec(policy):
        got, names = C.run_conv0(case, DEV)
    assert names == case.expected_launches(policy), names
    _compare(case, got, case.reference(), policy, "Conv0Im2col " + policy, ("y", "dw", "db", "dgray"))


# ---- the kernels only these layers call, directly --------------------------------------------------------------------------------
TAIL = 64


@pytest.mark.parametrize("shape", C.COL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_im2col3x3_c1_is_unfold(shape):
    """bit for bit F.unfold in columns 0..8, exact zeros in 9..11, nothing written past N H W 12"""
    from tpgsr_amd import kernels as K
    N, H, W = shape
    P = N * H * W
    gray, want = C.im2col_case(N, H, W)
    buf = torch.full((P * 12 + TAIL,), float("nan"), device=DEV)
    K.im2col3x3_c1(gray.to(DEV).contiguous(), N, H, W, buf)
    torch.cuda.synchronize()
    buf = buf.cpu()
    col = buf[:P * 12].view(P, 12)
    assert torch.equal(col[:, :9], want)
    assert torch.equal(col[:, 9:], torch.zeros(P, 3)) and not bool(torch.signbit(col[:, 9:]).any())
    assert bool(torch.isnan(buf[P * 12:]).all())


@pytest.mark.parametrize("shape", C.COL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_col2im3x3_c1_vs_fp64_adjoint(shape):
    """the adjoint of im2col over columns 0..8; non-zero garbage in columns 9..11 must not enter"""
    from tpgsr_amd import kernels as K
    N, H, W = shape
    dcol, r64, r32 = C.col2im_case(N, H, W)
    out = torch.full((N * H * W + TAIL,), float("nan"), device=DEV)
    K.col2im3x3_c1(dcol.to(DEV).contiguous(), N, H, W, out)
    torch.cuda.synchronize()
    out = out.cpu()
    assert bool(torch.isnan(out[N * H * W:]).all())
    e, bound = C.err(out[:N * H * W].view(N, 1, H, W), r64), C.arith_bound(r32, r64)
    WORST["col2im"] = max(WORST.get("col2im", 0.0), e / bound)
    print(f"col2im {shape}: e {e:.2e}  bound {bound:.2e}  ratio {e / bound:.2f}")
    assert e <= bound, (shape, e, bound)


@pytest.mark.parametrize("shape", C.PAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pad_channels_bit_for_bit(shape):
    from tpgsr_amd import kernels as K
    M, Cs, Cd = shape
    src, want = C.pad_case(M, Cs, Cd)
    buf = torch.full((M * Cd + TAIL,), float("nan"), device=DEV)
    K.pad_channels(src.to(DEV).contiguous(), M, Cs, Cd, buf)
    torch.cuda.synchronize()
    buf = buf.cpu()
    assert torch.equal(buf[:M * Cd].view(M, Cd), want) and not bool(torch.signbit(buf[:M * Cd].view(M, Cd)[:, Cs:]).any())
    assert bool(torch.isnan(buf[M * Cd:]).all())


def test_zz_report():
    for tag in sorted(WORST):
        print(f"engine CRNN layers {tag}: worst e / bound {WORST[tag]:.2f}")
