"""Shared by tests/test_loss_optim_ops_gpu.py and tests/test_metric_decode_ops_gpu.py: the case record and the error rule for kernels
that are called directly (tpgsr_amd.kernels / the loss modules), next to the `Case` table of tests/test_functional_ops_gpu.py whose
`_gen` / `err` / constants are used as they are.

A case is built on the CPU from a seeded generator: `make(seed)` returns its inputs (fp32 / int32 CPU tensors; seed 0 is the case
itself), `ref(d)` computes every output AND every gradient with stock PyTorch in the dtype of d's float tensors (called in float64 for
the reference, in float32 for e_ref32), `gpu(d)` runs the kernels on device copies and returns the same keys.

The rule, per key:
  exact    integer outputs and pure data movement: torch.equal against the float64 reference cast to the output's dtype.
  tensors  e_gpu <= 4 * e_ref32 + 4 * 2^-24 (the `arith` rule of the functional table), e = max |got - ref64| / max |ref64|.
  scalars  (loss values, norms, PSNR, mean SSIM, per-sample nll) the same rule with e_ref32 = the maximum over SCALAR_SEEDS seeds of the
           float32-CPU error at the case's shape: one scalar's float32 error is a lottery.
  caps     on top of either: the relative limit the kernel's fixture test already asserts (`caps`), or an absolute one (`abs_caps`).
  extra    a family's own additive term (key -> f(float64 inputs)), derived next to the case from the kernel's arithmetic and the float64
           reference alone, where 4x is not the whole story (SSIM gradient: the cancellation of its three addends).
Nothing in a bound comes from the GPU result."""
import math

import torch

from test_functional_ops_gpu import DEV, F64, FLOOR, MARGIN, _gen, err  # noqa: F401  (re-exported)

SCALAR_SEEDS = 8


class KCase:
    def __init__(self, family, name, make, ref, gpu, *, scalars=(), exact=(), caps=None, abs_caps=None, extra=None, margin=None, big=False):
        self.family, self.name, self.make, self.ref, self.gpu = family, name, make, ref, gpu
        self.scalars, self.exact, self.caps, self.abs_caps = tuple(scalars), tuple(exact), dict(caps or {}), dict(abs_caps or {})
        self.margin, self.big, self.extra, self._extra = margin, big, dict(extra or {}), {}
        self.id = f"{family}-{name}"
        self.ins = make(0)
        self._e32 = None


def cast(ins, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in ins.items()}


def reference(case, dtype, seed=0):
    ins = case.ins if seed == 0 else case.make(seed)
    return {k: v.detach() for k, v in case.ref(cast(ins, dtype)).items()}


def scalar_e32(case):
    """key -> max over the seeds of the float32-CPU error against float64 (the reference alone)"""
    if case._e32 is None:
        out = {k: 0.0 for k in case.scalars}
        for seed in range(SCALAR_SEEDS):
            r64, r32 = reference(case, F64, seed), reference(case, torch.float32, seed)
            for k in case.scalars:
                out[k] = max(out[k], err(r32[k], r64[k]))
        case._e32 = out
    return case._e32


def run_gpu(case):
    d = {k: (v.to(DEV).contiguous() if torch.is_tensor(v) else v) for k, v in case.ins.items()}
    got = {k: v.detach().cpu() for k, v in case.gpu(d).items()}
    torch.cuda.synchronize()
    return got


def bound_of(case, key, r32, r64):
    e32 = scalar_e32(case)[key] if key in case.scalars else err(r32[key], r64[key])
    b = 4 * e32 + FLOOR
    if key in case.extra:
        if key not in case._extra:
            case._extra[key] = float(case.extra[key](cast(case.ins, F64)))
        b += case._extra[key]
    return (min(b, case.caps[key]) if key in case.caps else b), e32


def check_well_posed(case):
    """CPU: margins, input sizes, a finite float64 reference with every key, a finite e_ref32 (over the seeds for scalars)"""
    lim = (32 << 20) if case.big else (8 << 20)
    assert all(v.numel() * v.element_size() < lim for v in case.ins.values() if torch.is_tensor(v)), case.id
    assert all(v.dtype in (torch.float32, torch.int32, torch.int64) for v in case.ins.values() if torch.is_tensor(v)), case.id
    if case.margin is not None:
        case.margin(cast(case.ins, F64))
    r64, r32 = reference(case, F64), reference(case, torch.float32)
    assert set(r64) == set(r32) and r64, case.id
    assert set(case.scalars) | set(case.exact) | set(case.caps) | set(case.abs_caps) <= set(r64), (case.id, sorted(r64))
    for key in r64:
        assert r64[key].shape == r32[key].shape and torch.isfinite(r64[key].double()).all(), (case.id, key)
        if key in case.exact:
            assert torch.equal(r64[key].to(r32[key].dtype), r32[key]), (case.id, key)
            continue
        assert r64[key].dtype == F64 and r32[key].dtype == torch.float32, (case.id, key, r64[key].dtype, r32[key].dtype)
        b, e32 = bound_of(case, key, r32, r64)
        assert math.isfinite(e32) and b > 0, (case.id, key, e32)


def check_case(case, worst):
    r64, r32 = reference(case, F64), reference(case, torch.float32)
    got = run_gpu(case)
    assert set(got) == set(r64), (sorted(got), sorted(r64))
    for key in sorted(r64):
        tag = f"{case.id} {key}"
        assert tuple(got[key].shape) == tuple(r64[key].shape), (tag, tuple(got[key].shape), tuple(r64[key].shape))
        if key in case.exact:
            want = r64[key].to(got[key].dtype)
            same = torch.equal(got[key], want)
            print(f"{tag}: bit-exact {same}")
            assert same, f"{tag}: differs at {(got[key] != want).nonzero()[:4].tolist()}"
            continue
        e_gpu = err(got[key], r64[key])
        bound, e32 = bound_of(case, key, r32, r64)
        worst[case.family] = max(worst.get(case.family, 0.0), e_gpu / bound)
        print(f"{tag}: e_gpu {e_gpu:.2e}  e_ref32 {e32:.2e}  bound {bound:.2e}  ratio {e_gpu / bound:.2f}")
        if not e_gpu <= bound:
            d = (got[key].double() - r64[key]).abs().reshape(-1)
            at = int(d.argmax()) if d.numel() else 0
            raise AssertionError(f"{tag}: e_gpu {e_gpu:.3e} > {bound:.3e} (e_ref32 {e32:.3e}); worst flat element {at}: got "
                                 f"{got[key].reshape(-1)[at].item():.9g}, float64 {r64[key].reshape(-1)[at].item():.9g}")
        if key in case.abs_caps:
            a = (got[key].double() - r64[key]).abs().max().item()
            print(f"{tag}: max |got - ref64| {a:.2e} (absolute cap {case.abs_caps[key]:.0e})")
            assert a <= case.abs_caps[key], (tag, a)
