"""Engine protocol for a drop-in network written OPERATOR BY OPERATOR over tpgsr_amd.functional (every operator a HIP kernel with a
hand-written backward, torch autograd only chains them) -- and the recorded-plan execution of such a network.

`TPGSRTrainStep` / `FusedAdam` / `ArenaPool` talk to a text-prior generator through its engine (`bind`, `forward`, `backward`, `arena`):
this adapter gives the `--tpg OPT` recogniser (`tpgsr_amd.model.crnn.model.Model`, reference model/crnn/model.py:25-110; selected for the
same training loop by interfaces/super_resolution.py:77-80 / interfaces/base.py:681-756) that interface, so it is a first-class
student / teacher of the fused train step: its parameters live in the pooled flat arena (one gradient-exchange bucket, one fused
clip + Adam).

Two ways to run it:

* RECORDED (default, `TPGSR_OPT_RECORD=0` switches it off): the module's forward and the autograd backward are executed ONCE per
  (batch size, mode, slot) under `kernels.recording` -- every operator's launches land in a `Plan` instead of on the GPU, against
  buffers the plan keeps alive -- and from then on a forward or backward pass is one replay of that plan by the native executor
  (csrc/plan.cpp): no Python per operator, no autograd, weight gradients on the weight-gradient stream with ONE batched slab reduce,
  exactly like `CRNNEngine`'s hand-recorded plans.  What makes the trace complete: parameter gradients are accumulated into the arena
  by the operators' own kernels (`functional.grad_sinks`; every operator gets its destination from `functional._grad_dst`, none opts
  out), tensors with two consumers go through `functional.fork` (their gradients are summed by tpgsr_add), so autograd never runs an ATen kernel of its own that a replay would miss -- tests/test_opt_recorded_gpu.py
  compares replays on fresh inputs with the operator-by-operator run.
* operator by operator through autograd (the reference implementation of the above; gradients accumulated by autograd into the arena's
  `.grad` views).

`FunctionalSREngine` (below) is the same adapter on the SR-network side of the protocol, for the `_TL` baseline backbones of the cascade loop
(`TPGSR_SR_RECORD=0` switches ITS recording off); `PlainSREngine` is that adapter for the prior-free baselines (SRResNet / RDN / VDSR).
The trace (`FunctionalEngine._trace`) and the two replays (`_replay_forward` / `_replay_backward`) exist once: a subclass names its static
inputs, its plans and its output, and keeps the operator-by-operator mode of its own `forward` / `backward`."""
import os
from typing import Dict, Optional

import torch

from . import functional as Fh
from . import kernels as K
from .engine import ParamArena
from .kernels import Plan, recording


class FunctionalEngine:
    FUSED = False        # no fused autograd node: tpgsr_amd.distributed.DataParallel hooks the parameters instead
    T, IMG_HW = 26, (32, 100)
    # what a recorded plan dictionary of this engine holds next to the static inputs (_static_inputs):
    PLAN_NAMES = ("opt_fwd", "opt_bwd")
    OUT, DOUT = "logits", "dlogits"      # the recorded output and the buffer its incoming gradient is copied into
    GRAD_OF = ("gray", "dgray")          # the static input whose gradient the backward plan leaves behind, and under which key (None: none)

    def __init__(self, module: torch.nn.Module):
        self.module = module
        self.arena = ParamArena(module)
        self.device = None
        self.record = os.environ.get("TPGSR_OPT_RECORD", "1") != "0"
        self._plans: Dict[tuple, dict] = {}      # _key() -> recorded plans + their static buffers
        self._saved: Dict[int, tuple] = {}
        self._pending_batches = 0
        self._kernel_writes = 0      # bumped by FusedAdam / broadcasts (engine protocol); every plan here re-packs its weights per replay

    def invalidate_packed(self):
        """engine protocol (engine._EngineBase.invalidate_packed): every plan here re-packs its weights per replay, so only the counter moves"""
        self._kernel_writes += 1

    def bind(self, device):
        rebuilt = self.arena.ensure(device)
        if rebuilt or self.device != device:
            for name, b in self.module.named_buffers():
                if b.device != device:
                    raise RuntimeError(f"buffer {name} is on {b.device}, parameters on {device}: call module.to(device) first")
            self._saved.clear()
            self._plans.clear()       # recorded against the old parameter / gradient addresses
        self.device = device

    def flush_counters(self):
        """BatchNorm's num_batches_tracked of the replays since the last flush (a recorded forward does not touch the counters)"""
        if self._pending_batches:
            for name, b in self.module.named_buffers():
                if name.endswith("num_batches_tracked"):
                    b += self._pending_batches
        self._pending_batches = 0

    def _check_mode(self, training):
        if bool(self.module.training) != bool(training):
            raise RuntimeError(f"{type(self.module).__name__}: forward(training={training}) on a module in "
                               f"{'train' if self.module.training else 'eval'}() mode")

    def _pop_saved(self, slot):
        if slot not in self._saved:
            raise RuntimeError(f"{type(self.module).__name__}: backward without a training-mode forward in slot {slot}")
        return self._saved.pop(slot)

    # ---- what a subclass describes --------------------------------------------------------------------------------------------------
    def _static_inputs(self, shape) -> dict:
        """the plan's input buffers, in the order the module takes them (shape: the first input's)"""
        return dict(gray=torch.empty(shape[0], 1, *self.IMG_HW, device=self.device))

    def _key(self, shape, training, slot, role) -> tuple:
        return (shape[0], bool(training), slot, role, K.POLICY)

    def _output(self, y):
        return y.permute(1, 0, 2)                        # [N][T][C]: the contiguous tensor the prediction layer wrote

    def _input_grad(self, got):
        return got[0] if got else None

    # ---- recorded mode ------------------------------------------------------------------------------------------------------------
    def _plans_for(self, shape, training: bool, slot: int = 0) -> dict:
        role = getattr(self, "role", "tpg")
        key = self._key(tuple(shape), training, slot, role)
        pl = self._plans.get(key)
        if pl is None:
            pl = self._plans[key] = self._trace(tuple(shape), training, role)
        return pl

    def _trace(self, shape, training, role):
        ins = self._static_inputs(shape)
        fwd = Plan(self.PLAN_NAMES[0])
        out = dict(fwd=fwd, **ins)
        x = ins[self.GRAD_OF[0]].requires_grad_(True) if training and self.GRAD_OF else None     # (the static buffer itself)
        with recording(fwd), K.conv_terms(K.terms_for(role, "fwd")), (torch.enable_grad() if training else torch.no_grad()):
            y = self.module(*ins.values())
        res = self._output(y)
        assert res.is_contiguous() and res.shape[0] == shape[0]
        out[self.OUT] = res.detach()
        if not training:
            return out
        bwd = K.backward_plan(self.PLAN_NAMES[1])
        dres = torch.empty_like(out[self.OUT])
        self.arena.attach_grads()
        grads = {p.data_ptr(): p.grad for p in self.module.parameters() if p.requires_grad}
        got = []
        h = x.register_hook(got.append) if x is not None else None
        try:
            # terms_for(role, "bwd"): for the recogniser the number "tpg" gives -- terms_for maps "teacher" to "tpg" outside the x2 policy
            # and returns 2 for either inside it
            with Fh.grad_sinks(grads), recording(bwd), K.conv_terms(K.terms_for(role, "bwd")):
                torch.autograd.backward(res, dres)
                if bwd.deferred is not None:
                    K.flush_wgrad_reduces()
                K._REC.join()
        finally:
            if h is not None:
                h.remove()
        out.update({"bwd": bwd, self.DOUT: dres})
        if x is not None:
            x.grad = None                                 # (assigned by autograd at trace time; the hook's tensor is the live one)
            out[self.GRAD_OF[1]] = self._input_grad(got)
        out["graph"] = y                                  # keeps the saved activations alive
        return out

    def _replay_forward(self, ins: dict, training, slot) -> torch.Tensor:
        """ins: the tensors for _static_inputs' buffers, in their order (None: zeros)"""
        first = next(iter(ins.values()))
        pl = self._plans_for(first.shape, training, slot)
        for name, t in ins.items():
            if t is None:
                K.zero(pl[name], pl[name].numel())
            else:
                K.copy(t.contiguous(), pl[name], t.numel())
        pl["fwd"].run()
        if training:
            self._pending_batches += 1
            self._saved[slot] = (first.shape[0], pl)
        res = torch.empty_like(pl[self.OUT])
        K.copy(pl[self.OUT], res, res.numel())
        return res

    def _replay_backward(self, N, dout, slot) -> dict:
        """-> the slot's plan dictionary, its backward plan replayed on `dout`"""
        n = self._saved[slot][0] if slot in self._saved else N
        if n != N:      # (the slot's activations stay: the backward pass of the forward that owns them still runs)
            raise RuntimeError(f"{type(self.module).__name__}: backward for a batch of {N} in slot {slot}, whose activations were overwritten "
                               f"by a later training-mode forward of {n} in the same slot")
        n, pl = self._pop_saved(slot)
        self.arena.attach_grads()                       # (same addresses as at trace time: the arena does not move)
        K.copy(dout.contiguous(), pl[self.DOUT], pl[self.DOUT].numel())
        pl["bwd"].run()
        return pl

    # ---- the engine protocol --------------------------------------------------------------------------------------------------------
    def forward(self, gray: torch.Tensor, training: bool, slot: int = 0, late_stream=None, after_late=None) -> torch.Tensor:
        """gray (N, 1, 32, 100) -> logits [N][T][nclass] (batch-major, like CRNNEngine.forward; late_stream / after_late: CRNNEngine's
        protocol -- nothing is packed apart here, the callback runs first)"""
        if after_late is not None:
            after_late()
        self._check_mode(training)
        self.bind(gray.device)
        if self.record:
            return self._replay_forward(dict(gray=gray), training, slot)
        if not training:
            with torch.no_grad():
                y = self.module(gray)                     # (T, N, C), a permuted view of the contiguous [N][T][C] result
            return y.permute(1, 0, 2).contiguous()
        x = gray.detach().requires_grad_(True)            # later cascade stages ask for d gray
        with torch.enable_grad():
            y = self.module(x)
        logits = y.permute(1, 0, 2)
        self._saved[slot] = (x, logits)
        return logits.detach().contiguous()

    def backward(self, N: int, gray: torch.Tensor, dlogits: torch.Tensor, need_dgray: bool = False, slot: int = 0) -> Optional[torch.Tensor]:
        if self.record:
            pl = self._replay_backward(N, dlogits, slot)
            if not need_dgray:
                return None
            res = torch.empty_like(pl["dgray"])
            K.copy(pl["dgray"], res, res.numel())
            return res
        x, logits = self._pop_saved(slot)
        self.arena.attach_grads()
        torch.autograd.backward(logits, dlogits.reshape(logits.shape))
        return x.grad if need_dgray else None


class FunctionalSREngine(FunctionalEngine):
    """The SR-network side of the engine protocol (`TSRNEngine`'s: forward_pre / forward / backward with cascade slots) for a backbone
    written operator by operator: the `_TL` baselines of the reference's ABLATION_SET (`--arch srresnet_tl | rdn_tl | srcnn_tl | vdsr_tl`,
    model/{srresnet,rdn,srcnn,vdsr}.py), which interfaces/super_resolution.py:295-424 trains through the same cascade loop as TSRN_TL.
    `TPGSRTrainStep`, `FusedAdam`, `ArenaPool` and `TextSREvaluator` drive the module through this adapter; `module(x, prior)` under
    autograd keeps working on its own.

    RECORDED (default, `TPGSR_SR_RECORD=0` switches it off): one trace (`FunctionalEngine._trace`) per (N, H, W, training, slot, policy)
    -- the slot keeps the saved activations of each cascade stage apart: a shared SR net runs `stu_iter` forward passes before any
    backward pass.  A forward and a backward pass are one replay each: parameter gradients go through `functional.GRAD_SINK` into the
    arena, weight gradients run on the weight-gradient stream with one batched slab reduce, every multi-consumer tensor of the module's
    forward is a `functional.fork`.  Otherwise operator by operator through autograd: the reference implementation of the recorded mode."""
    role = "sr"
    scale = 2            # SR grid / LR grid: the operator-level backbones are built for the reference's x2 only; a module that
                         # chains x2 stages gives ITS engine instance the module's factor (model/lapsrn.py LapSRN._engine)
    PLAN_NAMES = ("sr_tl_fwd", "sr_tl_bwd")
    OUT, DOUT = "sr", "dsr"
    GRAD_OF = ("prior", "dprior")

    def __init__(self, module: torch.nn.Module):
        super().__init__(module)
        self.record = os.environ.get("TPGSR_SR_RECORD", "1") != "0"

    def _static_inputs(self, shape) -> dict:
        return dict(lr=torch.empty(*shape, device=self.device), prior=torch.empty(shape[0], 37, 1, 26, device=self.device))

    def _key(self, shape, training, slot, role) -> tuple:
        return (shape, bool(training), slot, K.POLICY)

    def _output(self, y):
        return y

    def _input_grad(self, got):
        if not got or not got[0].is_contiguous():
            raise RuntimeError(f"{type(self.module).__name__}: the traced backward pass produced no contiguous text-prior gradient")
        return got[0]

    # ---- the engine protocol --------------------------------------------------------------------------------------------------------
    def forward_pre(self, lr, training, slot: int = 0, defer_join: bool = False):
        """engine protocol: the prior-independent prologue `TSRNEngine` runs next to the text-prior generator.  Nothing here is worth
        splitting out (the first conv of these backbones is a fraction of a percent of the pass): a no-op"""
        return None

    def forward(self, lr, training, prior=None, slot: int = 0, defer_join: bool = False, pre_done: bool = False) -> torch.Tensor:
        """lr (N, C, H, W), prior (N, 37, 1, 26) or None (zeros) -> SR image (N, C, 2H, 2W)"""
        self._check_mode(training)
        self.bind(lr.device)
        N = lr.shape[0]
        if prior is not None and tuple(prior.shape) != (N, 37, 1, 26):
            raise ValueError(f"{type(self.module).__name__}: the text prior is (N, 37, 1, 26), got {tuple(prior.shape)}")
        if self.record:
            return self._replay_forward(dict(lr=lr, prior=prior), training, slot)
        with K.conv_terms(K.terms_for("sr", "fwd")):
            if not training:
                with torch.no_grad():
                    return self.module(lr, prior)
            t = (prior if prior is not None else torch.zeros(N, 37, 1, 26, device=lr.device)).detach().requires_grad_(True)
            with torch.enable_grad():
                y = self.module(lr.detach(), t)
        self._saved[slot] = (t, y)
        return y.detach()

    def backward(self, x_shape, sr, dsr, slot: int = 0, defer_join: bool = False) -> torch.Tensor:
        """d loss / d SR image -> d loss / d prior (N, 37, 1, 26); parameter gradients are accumulated into the arena"""
        if self.record:
            return self._replay_backward(x_shape[0], dsr, slot)["dprior"]    # the plan's buffer of this slot: valid until the slot's next backward pass
        t, y = self._pop_saved(slot)
        self.arena.attach_grads()
        with K.conv_terms(K.terms_for("sr", "bwd")):
            torch.autograd.backward(y, dsr.reshape(y.shape))
        return t.grad.contiguous()


class PlainSREngine(FunctionalSREngine):
    """`FunctionalSREngine` for a backbone WITHOUT a text prior: the reference's prior-free baselines (`--arch srres | rdn | vdsr | lapsrn | esrgan | edsr | srcnn`,
    model/{srresnet,rdn,vdsr,lapsrn,esrgan,edsr,srcnn}.py SRResNet / RDN / VDSR / LapSRN / RRDBNet / EDSR / SRCNN), which the `else:` branch of the train loop (interfaces/super_resolution.py:409-424)
    trains with `model(images_lr[:, :channel_num])`.  `SRTrainStep`, `FusedAdam`, `ArenaPool` and `TextSREvaluator` drive the module
    through this adapter; `module(x)` under autograd keeps working on its own.

    The same two modes: RECORDED (default, `TPGSR_SR_RECORD=0` switches it off) traces `module(lr)` once per (shape, training, slot,
    policy) into a forward and a backward plan -- parameter gradients through `functional.GRAD_SINK` into the arena, weight gradients on
    the weight-gradient stream with one batched slab reduce; otherwise operator by operator through autograd.  The input image needs no
    gradient, so the first layer's data gradient is never launched, and `backward` returns nothing."""
    PLAN_NAMES = ("sr_plain_fwd", "sr_plain_bwd")
    GRAD_OF = None

    def _static_inputs(self, shape) -> dict:
        return dict(lr=torch.empty(*shape, device=self.device))

    def forward(self, lr, training, prior=None, slot: int = 0, defer_join: bool = False, pre_done: bool = False) -> torch.Tensor:
        """lr (N, C, H, W) -> SR image (N, C, scale H, scale W)"""
        if prior is not None:
            raise ValueError(f"{type(self.module).__name__} takes no text prior")
        self._check_mode(training)
        self.bind(lr.device)
        if self.record:
            return self._replay_forward(dict(lr=lr), training, slot)
        with K.conv_terms(K.terms_for("sr", "fwd")):
            if not training:
                with torch.no_grad():
                    return self.module(lr)
            with torch.enable_grad():
                y = self.module(lr.detach())
        self._saved[slot] = (None, y)
        return y.detach()

    def backward(self, x_shape, sr, dsr, slot: int = 0, defer_join: bool = False) -> None:
        """d loss / d SR image -> parameter gradients, accumulated into the arena (there is no prior to return a gradient for)"""
        if self.record:
            self._replay_backward(x_shape[0], dsr, slot)
            return None
        _, y = self._pop_saved(slot)
        self.arena.attach_grads()
        with K.conv_terms(K.terms_for("sr", "bwd")):
            torch.autograd.backward(y, dsr.reshape(y.shape))
        return None
