"""GPU: engines, train steps and the evaluator under MIXED call sequences (tests/call_sequence_common.py) -- what outlives a call: the plan
caches keyed by batch size / mode / slot / policy, the scratch all plans of an engine share (regrown by a bigger batch while older plans
point into the old one), workspace slots, the packed-operand keys and the late split table, the pending BatchNorm counters, a train step's
static buffers and captured graphs, Adam's state and the pooled arenas.

HISTORY INDEPENDENCE, bit for bit: call k on a long-lived object equals the same call on a fresh twin loaded from a snapshot taken just
before it -- returned outputs, `last_sr`, the loss, the pooled parameter and gradient arenas, every buffer (num_batches_tracked after a
flush), Adam's m / v / step.  No tolerance appears: the suite already holds whole trajectories bitwise equal between replicas and between
eager and replayed steps (test_tsrn_gpu.py, test_crnn_gpu.py, test_plain_baselines_gpu.py, test_cascade_topology_gpu.py).  The one
exception is the accumulated gradient arena of the slots test, compared under the rule tests/test_fullsize_gpu.py already uses for it
(1e-6 of its largest magnitude): the two orders add the same two gradients in another order inside the weight-gradient kernels.

OUTPUTS ARE NOT ALIASED: every tensor a forward, an evaluator or a module call returned earlier in a sequence still equals its clone at
the end.  Exempt, because documented as static: the loss scalar of step() / replay() (a buffer of the step, rewritten by its next step at
that shape) and what a replay leaves in the captured graph's own memory (`last_sr` of a replay).

Batch sizes 4, 6, 1, 4 on LR 16x64 -> HR 32x128, distinct data per call."""
import gc
import weakref

import pytest
import torch

pytestmark = pytest.mark.gpu

import call_sequence_common as C  # noqa: E402

DEV = "cuda"


def _compare(k, op, A, out_a, B, out_b):
    torch.cuda.synchronize()
    tag = f"call {k} {op}"
    C.same_bits(out_a, out_b, tag + " returned")
    C.same_bits(C.state_bits(A, grads=op[0] not in ("eval", "evb")), C.state_bits(B, grads=op[0] not in ("eval", "evb")), tag + " state")


# ---- eval batch sizes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tsrn", "tsrn_tl", "crnn", "srres", "edsr"])
def test_eval_forward_at_each_batch_size_equals_a_fresh_module(name):
    """module(x) in eval mode at N = 4, 6, 1, 4 on ONE module: each equals a fresh module; all four returned tensors are intact at the end"""
    A = C.run_sequence(C.module_builder(name, DEV), C.EVAL_SEQ, DEV, _compare)
    if name in ("tsrn", "tsrn_tl", "crnn"):
        assert len(A[0]._engine()._plans) == 3


# ---- train steps with evaluation in between ---------------------------------------------------------------------------------------------
def _step_sequence(builder):
    A = C.run_sequence(builder, C.STEP_SEQ, DEV, _compare)
    # a second replica that makes ONLY the training calls ends in the same bits: the interleaved evaluation perturbed nothing
    R = builder()
    for op in C.training_only(C.STEP_SEQ):
        C.run_call(R, op, DEV)
    torch.cuda.synchronize()
    C.same_bits(C.state_bits(A), C.state_bits(R), "against the replica without evaluation")


@pytest.mark.parametrize("name", ["tsrn", "tsrn_stn"])
def test_tsrn_train_step_with_interleaved_eval(name):
    _step_sequence(C.step_builder(name, DEV))


@pytest.mark.parametrize("name", ["srres", "edsr", "rrdb"])
def test_sr_train_step_with_interleaved_eval(name):
    """srres: running statistics and the functional engine's pending batch counter; EDSR / RRDBNet with channels=3: lr_c / hr_c are rebuilt
    per shape, no BatchNorm, RRDBNet's dense-block buffers"""
    _step_sequence(C.step_builder(name, DEV))


# ---- the cascade and its evaluator --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stu_iter", [1, 2])
def test_cascade_steps_with_interleaved_evaluator(stu_iter):
    """TPGSRTrainStep at N = 4, 6, 4 (the benchmarked policy x2; stu_iter 2 with a shared SR network: its slots are reused by every step) and
    one long-lived TextSREvaluator over the same modules at N = 6 and N = 1 in between: strings, PSNR, SSIM, SR images and priors equal
    those of an evaluator over fresh modules"""
    C.run_sequence(C.cascade_builder(DEV, stu_iter, precision="x2"), C.CASCADE_SEQ, DEV, _compare)


# ---- policy changes on a live module ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tsrn", "crnn"])
@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
def test_policy_changes_on_a_live_module(name, training):
    """one live module under f32 FIRST (bound without bf16 twins: the split table is built late, when x2 records its first plan), then x2,
    x3, bf16 (both engines record it), f32 again: each run -- an eval forward, or a training forward and backward through autograd --
    equals a fresh module under that policy: output, gradient arena, running statistics and batch counters"""
    from tpgsr_amd import kernels as K
    builder = C.module_builder(name, DEV, training)
    A = builder()
    held = []

    def run(obj, k):
        args = C.MODULES[name][1](4, 50 + k, DEV)
        if not training:
            with torch.no_grad():
                return dict(y=obj[0](*args))
        eng = obj[0]._engine()
        eng.bind(torch.device(DEV, 0))
        eng.arena.attach_grads()
        eng.arena.grad.zero_()
        y = obj[0](*args)
        gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(60 + k)).to(DEV)
        (y * gy).sum().backward()
        return dict(y=y.detach())

    for k, pol in enumerate(C.POLICIES):
        snap = C.snapshot(A)
        with K.policy(pol):
            out_a = run(A, k)
            B = C.fresh_twin(snap, builder)
            out_b = run(B, k)
        held.append((f"{pol} y", out_a["y"], out_a["y"].clone()))
        _compare(k, ("train" if training else "eval", 4, pol), A, out_a, B, out_b)
    C.check_held(held)
    eng = A[0]._engine()
    assert len(eng._live) == 0 and len(eng._plans) == len(set(C.POLICIES))


# ---- slots: two outstanding forwards of different batch sizes ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tsrn", "srres"])
def test_module_api_two_shapes_outstanding(name):
    """forward N = 4, forward N = 6, backward of the second, backward of the first, through the nn.Module API: outputs bitwise those of the
    twin's sequential run (forward, backward, forward, backward), the accumulated gradient arena under the rule of
    tests/test_fullsize_gpu.py (1e-6 of its largest magnitude), running statistics bitwise (the forwards ran in the same order)"""
    builder = C.module_builder(name, DEV, True)
    A = builder()
    B = C.fresh_twin(C.snapshot(A), builder)
    xa, xb = C.MODULES[name][1](4, 91, DEV)[0], C.MODULES[name][1](6, 92, DEV)[0]
    ga, gb = [torch.randn(n, 4, 32, 128, generator=torch.Generator().manual_seed(s)).to(DEV) for n, s in ((4, 93), (6, 94))]
    for obj in (A, B):
        eng = obj[0]._engine()
        eng.bind(torch.device(DEV, 0))
        eng.arena.attach_grads()
        eng.arena.grad.zero_()
    ya = A[0](xa)
    ya_clone = ya.detach().clone()
    yb = A[0](xb)
    (yb * gb).sum().backward()
    (ya * ga).sum().backward()
    ra = B[0](xa)
    (ra * ga).sum().backward()
    rb = B[0](xb)
    (rb * gb).sum().backward()
    torch.cuda.synchronize()
    C.same_bits(dict(ya=ya.detach(), yb=yb.detach()), dict(ya=ra.detach(), yb=rb.detach()), "outputs")
    assert torch.equal(ya.detach(), ya_clone)
    C.same_bits(C.state_bits(A, grads=False), C.state_bits(B, grads=False), "buffers and parameters")
    got, ref = A[0]._engine().arena.grad, B[0]._engine().arena.grad
    d = float((got - ref).abs().max())
    print(f"{name}: accumulated gradients max diff {d:.3e} of {float(ref.abs().max()):.3e}")
    assert d <= 1e-6 * float(ref.abs().max())
    eng = A[0]._engine()
    assert len(getattr(eng, "_live", {})) == 0 and len(getattr(eng, "_saved", {})) == 0


@pytest.mark.parametrize("name", ["srres", "edsr"])
def test_functional_engine_slots_and_refusal(name):
    """engine protocol with explicit slots (what a cascade with a shared SR network does): forward N = 4 in slot 0, forward N = 6 in slot 1,
    backward slot 1, backward slot 0 -- gradients of each equal a fresh engine's; then a slot overwritten at another batch size: the stale
    backward raises the RuntimeError the TSRN engine gives for overwritten activations, the owner's backward still runs and equals a twin's"""
    builder = C.module_builder(name, DEV, True)
    A = builder()
    eng = A[0]._engine()
    x4, x6 = C.MODULES[name][1](4, 95, DEV)[0], C.MODULES[name][1](6, 96, DEV)[0]

    def dsr_for(sr, seed):
        return torch.randn(sr.shape, generator=torch.Generator().manual_seed(seed)).to(DEV)

    def fresh_grad(snap, x, seed):
        B = C.fresh_twin(snap, builder)
        e = B[0]._engine()
        sr = e.forward(x, True, slot=0)
        e.arena.attach_grads()
        e.arena.grad.zero_()
        e.backward(tuple(x.shape), sr, dsr_for(sr, seed), slot=0)
        torch.cuda.synchronize()
        return sr, e.arena.grad.clone()

    snap4 = C.snapshot(A)
    sr4 = eng.forward(x4, True, slot=0)
    snap6 = C.snapshot(A)
    sr6 = eng.forward(x6, True, slot=1)
    for sr, x, snap, slot, seed in ((sr6, x6, snap6, 1, 98), (sr4, x4, snap4, 0, 97)):
        eng.arena.attach_grads()
        eng.arena.grad.zero_()
        eng.backward(tuple(x.shape), sr, dsr_for(sr, seed), slot=slot)
        torch.cuda.synchronize()
        ref_sr, ref_grad = fresh_grad(snap, x, seed)
        C.same_bits(dict(sr=sr, grad=eng.arena.grad), dict(sr=ref_sr, grad=ref_grad), f"slot {slot}")
    assert len(eng._saved) == 0
    # the refusal
    sr4 = eng.forward(x4, True, slot=0)
    snap6 = C.snapshot(A)
    sr6 = eng.forward(x6, True, slot=0)
    with pytest.raises(RuntimeError, match="overwritten"):
        eng.backward(tuple(x4.shape), sr4, dsr_for(sr4, 97), slot=0)
    eng.arena.attach_grads()
    eng.arena.grad.zero_()
    eng.backward(tuple(x6.shape), sr6, dsr_for(sr6, 98), slot=0)
    torch.cuda.synchronize()
    ref_sr, ref_grad = fresh_grad(snap6, x6, 98)
    C.same_bits(dict(sr=sr6, grad=eng.arena.grad), dict(sr=ref_sr, grad=ref_grad), "owner of the slot")
    assert len(eng._saved) == 0


# ---- capture, then another shape ------------------------------------------------------------------------------------------------------------
def _static_tensors(st):
    return [(k, t) for k, v in st.items() for t in (v if isinstance(v, list) else [v]) if isinstance(t, torch.Tensor)]


@pytest.mark.parametrize("name", ["srres", "cascade"])
def test_capture_then_another_shape(name):
    """capture at N = 4, replay, an eager step at N = 6 (the ragged last batch), replay with new N = 4 data, an eager step at N = 4.  The
    captured graph holds the addresses of the static set of ITS shape (dloss = 100.0 scales every gradient): BEFORE the first replay that
    follows the eager N = 6 step, every tensor of that set must still be referenced -- asserted on the host, so a step that released them
    never replays on released buffers.  Then every replay and step equals the eager twin's step, bitwise."""
    builder = C.cascade_builder(DEV, 1, precision="x2") if name == "cascade" else C.step_builder("srres", DEV)
    A = builder()
    held, refs = [], None
    for k, op in enumerate(C.CAPTURE_SEQ):
        if op[0] == "replay" and k > 1:
            gc.collect()
            dead = sorted({key for key, r in refs if r() is None})
            assert not dead, f"static buffers of the captured shape were released by the eager step at another shape: {dead}"
        snap = C.snapshot(A)
        out_a = C.run_call(A, op, DEV, held)
        if op[0] == "capture":
            refs = [(key, weakref.ref(t)) for key, t in _static_tensors(A._static)]
            assert len(refs) >= 5 and tuple(A._static.get("shape", A._static.get("key", (None, None))[1])) == (4, 4, 16, 64)
        B = C.fresh_twin(snap, builder)
        out_b = C.run_call(B, C.twin_op(op), DEV)
        if op[0] == "capture":      # (the capture executes nothing: its `last_sr` is unwritten graph memory; the warm-up step's loss and state are compared)
            out_b = {key: out_b[key] for key in out_a}
        _compare(k, op, A, out_a, B, out_b)
        if op[0] == "step":
            assert A._static["loss"] is not None and tuple(A._static.get("shape", A._static.get("key", (None, None))[1]))[0] == op[1]
    C.check_held(held)
