"""The 64-unit bidirectional GRU (`Fh.bigru` with weight_hh_l0 [192][64]: csrc/gru.hip, bigru_fwd_kernel<64> / bigru_bwd_kernel<64>) against
torch.nn.GRU(Cin, 64, bidirectional=True, batch_first=True) in float64 on the CPU, element by element.

Method and bounds are those of tests/test_functional_ops_gpu.py (its Case record, run_reference / run_gpu / err and CONV_LIMITS are imported,
not restated): random upstream gradient, h, dx, dW_ih, db_ih, dW_hh, db_hh compared over the whole tensor with
e = max |got - ref| / max |ref|, contiguous and non-contiguous inputs, bounds 5e-6 / 1e-5 under "x3" and 2e-5 / 2e-5 under "x2".

Shapes (N, H, W), each along W (axis 0) and along H (axis 1), are the smallest that reach every branch of the scan (PF = prefetch depth, 8):
  (1,1,1)   T = 1: the initial state only            (2,3,5)   T < PF, the bounds-tested (non-EXACT) kernel
  (1,2,8) and (1,8,2)   T = PF: EXACT, one group     (2,16,9)  T = 16 EXACT on one axis, T = 9 non-EXACT across a ring refill on the other
  (1,2,24)  three groups
with Cin 128 and 160: the two GruBlocks of a TSRN_TL block at hidden_units = 64 (C and C + 32).

Observed on an MI355X, worst e / bound over all cases (`test_zz_report` prints it): x3 0.05, x2 0.64 (the 32-unit cases of
tests/test_functional_ops_gpu.py: 0.05 and 0.71); with the prefetch depth at 4 and at 12 (x3): 0.05.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_functional_ops_gpu as T  # noqa: E402

U = 64
SHAPES = [(1, 1, 1), (2, 3, 5), (1, 2, 8), (1, 8, 2), (2, 16, 9), (1, 2, 24)]
CINS = (128, 160)


def _gru_ref(d, axis):
    x = d["x"]
    N, H, W, Cin = x.shape
    if axis == 0:
        return T._rnn_ref(torch.nn.GRU, x.reshape(N * H, W, Cin), d, U).reshape(N, H, W, 2 * U)
    return T._rnn_ref(torch.nn.GRU, x.permute(0, 2, 1, 3).reshape(N * W, H, Cin), d, U).reshape(N, W, H, 2 * U).permute(0, 2, 1, 3)


def _cases():
    from tpgsr_amd import functional as Fh
    out = []
    for axis in (0, 1):
        for N, H, W in SHAPES:
            for Cin in CINS:
                g = T._gen("bigru64", axis, N, H, W, Cin)
                ins = {"x": torch.randn(N, H, W, Cin, generator=g), **T._rnn_params(g, Cin, U, 3)}
                out.append(T.Case("bigru64", f"axis{axis}-{N}x{H}x{W}-C{Cin}", "conv", ins, ["x"], list(ins), lambda d, a=axis: _gru_ref(d, a),
                                  lambda d, a=axis: Fh.bigru(d["x"], T._gru_holder(d), a), shape=(N, H, W, 2 * U)))
    return out


CASES = _cases()
_REF = {}
WORST = {}


def _ref64(case):
    """the float64 reference of a case, computed once and shared by every test that needs it (never modified)"""
    if case.id not in _REF:
        _REF[case.id] = T.run_reference(case, T.F64)
    return _REF[case.id]


def _check(case, policy, tag, passes=(False, True)):
    r64 = _ref64(case)
    assert tuple(r64["y0"].shape) == case.shape
    for nc in passes:
        got = T.run_gpu(case, nc)
        assert set(got) == set(r64), (sorted(got), sorted(r64))
        for key in sorted(r64):
            assert tuple(got[key].shape) == tuple(r64[key].shape), key
            is_par = key.startswith("d") and key[1:] not in case.acts
            bound = T.CONV_LIMITS[policy][1 if is_par else 0]
            e = T.err(got[key], r64[key])
            WORST[tag] = max(WORST.get(tag, 0.0), e / bound)
            print(f"{case.id}-{tag} [{'non-contiguous' if nc else 'contiguous'}] {key}: e_gpu {e:.2e}  bound {bound:.2e}  ratio {e / bound:.2f}")
            assert e <= bound, f"{case.id}-{tag} nc={nc} {key}: e_gpu {e:.3e} > {bound:.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("policy", ["x3", "x2"])
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_bigru64_vs_fp64(case, policy):
    from tpgsr_amd import kernels as K
    prev = K.POLICY
    K.set_conv_prec(policy)
    try:
        _check(case, policy, policy)
    finally:
        K.set_conv_prec(prev)


@pytest.mark.gpu
@pytest.mark.parametrize("pf", [4, 12])
def test_bigru64_other_prefetch_depths(pf):
    """the same shapes with the look-ahead of the operand rings set to 4 and to 12 (tpgsr_gru_set_prefetch; the 64-unit scans run 12 as 8)"""
    from tpgsr_amd import _lib, kernels as K
    prev = K.POLICY
    K.set_conv_prec("x3")
    _lib.load().tpgsr_gru_set_prefetch(pf)
    try:
        for case in CASES:
            _check(case, "x3", f"x3-pf{pf}", passes=(False,))
    finally:
        _lib.load().tpgsr_gru_set_prefetch(8)
        K.set_conv_prec(prev)


def _raw(N, H, W, axis, seed):
    """one raw forward + backward launch pair on seeded operands: (h, gates, dgi, dgh)"""
    from tpgsr_amd import kernels as K
    g = torch.Generator().manual_seed(seed)
    P = N * H * W
    r = lambda *s: (torch.rand(*s, generator=g) * 2 - 1).cuda()
    gi, whh, bhh, dh = r(P, 6 * U), r(2, 3 * U, U) / 8, r(2, 3 * U) / 8, r(P, 2 * U)
    h, gates = torch.empty(P, 2 * U, device="cuda"), torch.empty(P, 8 * U, device="cuda")
    dgi, dgh = torch.empty(P, 6 * U, device="cuda"), torch.empty(P, 6 * U, device="cuda")
    K.bigru_fwd(gi, whh, bhh, N, H, W, axis, h, gates, hidden=U)
    K.bigru_bwd(gates, h, dh, None, whh, N, H, W, axis, dgi, dgh, hidden=U)
    torch.cuda.synchronize()
    return h, gates, dgi, dgh


@pytest.mark.gpu
@pytest.mark.parametrize("axis", [0, 1])
def test_bigru64_two_launches_are_bitwise_equal(axis):
    a, b = _raw(2, 16, 9, axis, 7), _raw(2, 16, 9, axis, 7)
    for x, y, name in zip(a, b, ("h", "gates", "dgi", "dgh")):
        assert torch.equal(x, y), name


@pytest.mark.gpu
def test_bigru64_inference_form_and_second_gradient():
    """gates = NULL (inference) gives the same h; dh_out2 is added to dh_out (the engine's two gradient paths into a block)"""
    from tpgsr_amd import kernels as K
    N, H, W, axis = 2, 3, 9, 0
    g = torch.Generator().manual_seed(11)
    P = N * H * W
    r = lambda *s: (torch.rand(*s, generator=g) * 2 - 1).cuda()
    gi, whh, bhh, dh, dh2 = r(P, 6 * U), r(2, 3 * U, U) / 8, r(2, 3 * U) / 8, r(P, 2 * U), r(P, 2 * U)
    h, h_inf, gates = torch.empty(P, 2 * U, device="cuda"), torch.empty(P, 2 * U, device="cuda"), torch.empty(P, 8 * U, device="cuda")
    K.bigru_fwd(gi, whh, bhh, N, H, W, axis, h, gates, hidden=U)
    K.bigru_fwd(gi, whh, bhh, N, H, W, axis, h_inf, None, hidden=U)
    assert torch.equal(h, h_inf)
    out = [[torch.empty(P, 6 * U, device="cuda") for _ in range(2)] for _ in range(2)]
    K.bigru_bwd(gates, h, dh, dh2, whh, N, H, W, axis, *out[0], hidden=U)
    K.bigru_bwd(gates, h, dh + dh2, None, whh, N, H, W, axis, *out[1], hidden=U)
    torch.cuda.synchronize()
    for a, b in zip(out[0], out[1]):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_bigru64_refusals_and_the_32_unit_path():
    from tpgsr_amd import functional as Fh, kernels as K, _lib
    g = T._gen("bigru64-refusals")
    # U = 48: refused by the host, nothing launched (no kernel error, the message names the supported sizes)
    p = {k: v.cuda() for k, v in T._rnn_params(g, 64, 48, 3).items()}
    with pytest.raises(NotImplementedError, match="32 or 64"):
        Fh.bigru(torch.randn(1, 2, 3, 64, device="cuda"), T._gru_holder(p), 0)
    with pytest.raises(NotImplementedError, match="32 or 64"):
        K.bigru_fwd(None, None, None, 1, 2, 3, 0, None, None, hidden=48)
    # ... and by the C ABI, as an argument error
    z = torch.zeros(8 * 6 * 48, device="cuda")
    rc = _lib.load().tpgsr_bigru_fwd_u(z.data_ptr(), z.data_ptr(), z.data_ptr(), 1, 2, 3, 0, 48, z.data_ptr(), None, None)
    assert rc != 0
    # the index bound: N H W 8U < 2^31
    rc = _lib.load().tpgsr_bigru_fwd_u(z.data_ptr(), z.data_ptr(), z.data_ptr(), 4096, 32, 32, 0, 64, z.data_ptr(), None, None)
    assert rc != 0
    # U = 32 through Fh.bigru: bitwise what the tpgsr_bigru_fwd path gives on the same projection
    N, H, W, Cin = 2, 3, 9, 64
    p = {k: v.cuda() for k, v in T._rnn_params(g, Cin, 32, 3).items()}
    x = torch.randn(N, H, W, Cin, generator=g).cuda()
    hold = T._gru_holder(p)
    with torch.no_grad():
        h = Fh.bigru(x, hold, 0)
        gi = Fh._GruProj.apply(x, hold.weight_ih_l0, hold.weight_ih_l0_reverse, hold.bias_ih_l0, hold.bias_ih_l0_reverse)
    whh = torch.stack([p["w_hh"], p["w_hh_r"]]).contiguous()
    bhh = torch.stack([p["b_hh"], p["b_hh_r"]]).contiguous()
    h0 = torch.empty(N, H, W, 64, device="cuda")
    K.bigru_fwd(gi.contiguous(), whh, bhh, N, H, W, 0, h0, None)
    h1 = torch.empty_like(h0)
    rc = _lib.load().tpgsr_bigru_fwd_u(gi.data_ptr(), whh.data_ptr(), bhh.data_ptr(), N, H, W, 0, 32, h1.data_ptr(), None,
                                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(h, h0) and torch.equal(h1, h0)


@pytest.mark.gpu
def test_zz_report():
    for tag in sorted(WORST):
        print(f"bigru64 {tag}: worst e_gpu / bound {WORST[tag]:.2f}")
