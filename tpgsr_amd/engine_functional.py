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
  by the operators' own kernels (`functional.GRAD_SINK`), tensors with two consumers go through `functional.fork` (their gradients are
  summed by tpgsr_add), so autograd never runs an ATen kernel of its own that a replay would miss -- tests/test_opt_recorded_gpu.py
  compares replays on fresh inputs with the operator-by-operator run.
* operator by operator through autograd (the reference implementation of the above; gradients accumulated by autograd into the arena's
  `.grad` views).

`FunctionalSREngine` (below) is the same adapter on the SR-network side of the protocol, for the `_TL` baseline backbones of the cascade loop
(`TPGSR_SR_RECORD=0` switches ITS recording off); `PlainSREngine` is that adapter for the prior-free baselines (SRResNet / RDN / VDSR)."""
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

    def __init__(self, module: torch.nn.Module):
        self.module = module
        self.arena = ParamArena(module)
        self.device = None
        self.record = os.environ.get("TPGSR_OPT_RECORD", "1") != "0"
        self._plans: Dict[tuple, dict] = {}      # (N, training, slot, role) -> recorded plans + their static buffers
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

    # ---- recorded mode ------------------------------------------------------------------------------------------------------------
    def plans(self, N: int, training: bool, slot: int = 0) -> dict:
        role = getattr(self, "role", "tpg")
        key = (N, bool(training), slot, role, K.POLICY)
        pl = self._plans.get(key)
        if pl is None:
            pl = self._plans[key] = self._trace(N, training, role)
        return pl

    def _trace(self, N, training, role):
        dev = self.device
        gray = torch.empty(N, 1, *self.IMG_HW, device=dev)
        fwd = Plan("opt_fwd")
        out = dict(fwd=fwd, gray=gray)
        with recording(fwd), K.conv_terms(K.terms_for(role, "fwd")):
            if training:
                x = gray.requires_grad_(True)
                with torch.enable_grad():
                    y = self.module(x)
            else:
                with torch.no_grad():
                    y = self.module(gray)
        logits = y.permute(1, 0, 2)                      # [N][T][C]: the contiguous tensor the prediction layer wrote
        assert logits.is_contiguous() and logits.shape[0] == N
        out["logits"] = logits
        if not training:
            return out
        bwd = Plan("opt_bwd")
        bwd.overlap = os.environ.get("TPGSR_OVERLAP_WGRAD", "1") != "0"
        bwd.deferred = [] if os.environ.get("TPGSR_DEFER_REDUCE", "1") != "0" else None
        dlogits = torch.empty_like(logits)
        self.arena.attach_grads()
        grads = {p.data_ptr(): p.grad for p in self.module.parameters() if p.requires_grad}
        got = []
        h = x.register_hook(lambda g_: got.append(g_))
        prev, Fh.GRAD_SINK = Fh.GRAD_SINK, grads
        try:
            with recording(bwd), K.conv_terms(K.terms_for("tpg", "bwd")):
                torch.autograd.backward(logits, dlogits)
                if bwd.deferred is not None:
                    K.flush_wgrad_reduces()
                K._REC.join()
        finally:
            Fh.GRAD_SINK = prev
            h.remove()
        x.grad = None                                     # (assigned by autograd at trace time; the hook's tensor is the live one)
        out.update(bwd=bwd, dlogits=dlogits, dgray=got[0] if got else None, graph=y)     # `graph` keeps the saved activations alive
        return out

    # ---- the engine protocol --------------------------------------------------------------------------------------------------------
    def forward(self, gray: torch.Tensor, training: bool, slot: int = 0, late_stream=None, after_late=None) -> torch.Tensor:
        """gray (N, 1, 32, 100) -> logits [N][T][nclass] (batch-major, like CRNNEngine.forward; late_stream / after_late: CRNNEngine's
        protocol -- nothing is packed apart here, the callback runs first)"""
        if after_late is not None:
            after_late()
        if bool(self.module.training) != bool(training):
            raise RuntimeError(f"{type(self.module).__name__}: forward(training={training}) on a module in "
                               f"{'train' if self.module.training else 'eval'}() mode")
        self.bind(gray.device)
        if self.record:
            N = gray.shape[0]
            pl = self.plans(N, training, slot)
            K.copy(gray.contiguous(), pl["gray"], gray.numel())
            pl["fwd"].run()
            if training:
                self._pending_batches += 1
                self._saved[slot] = (N, pl)
            res = torch.empty_like(pl["logits"])
            K.copy(pl["logits"], res, res.numel())
            return res
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
        if slot not in self._saved:
            raise RuntimeError(f"{type(self.module).__name__}: backward without a training-mode forward in slot {slot}")
        if self.record:
            n, pl = self._saved.pop(slot)
            assert n == N
            self.arena.attach_grads()                       # (same addresses as at trace time: the arena does not move)
            K.copy(dlogits.contiguous(), pl["dlogits"], pl["dlogits"].numel())
            pl["bwd"].run()
            if not need_dgray:
                return None
            res = torch.empty_like(pl["dgray"])
            K.copy(pl["dgray"], res, res.numel())
            return res
        x, logits = self._saved.pop(slot)
        self.arena.attach_grads()
        torch.autograd.backward(logits, dlogits.reshape(logits.shape))
        return x.grad if need_dgray else None


class FunctionalSREngine(FunctionalEngine):
    """The SR-network side of the engine protocol (`TSRNEngine`'s: forward_pre / forward / backward with cascade slots) for a backbone
    written operator by operator: the `_TL` baselines of the reference's ABLATION_SET (`--arch srresnet_tl | rdn_tl | srcnn_tl | vdsr_tl`,
    model/{srresnet,rdn,srcnn,vdsr}.py), which interfaces/super_resolution.py:295-424 trains through the same cascade loop as TSRN_TL.
    `TPGSRTrainStep`, `FusedAdam`, `ArenaPool` and `TextSREvaluator` drive the module through this adapter; `module(x, prior)` under
    autograd keeps working on its own.

    RECORDED (default, `TPGSR_SR_RECORD=0` switches it off): one trace per (N, H, W, training, slot, policy) -- the slot keeps the saved
    activations of each cascade stage apart: a shared SR net runs `stu_iter` forward passes before any backward pass.  A forward and a
    backward pass are one replay each: parameter gradients go through `functional.GRAD_SINK` into the arena, weight gradients run on the
    weight-gradient stream with one batched slab reduce, every multi-consumer tensor of the module's forward is a `functional.fork`.
    Otherwise operator by operator through autograd: the reference implementation of the recorded mode."""
    FUSED = False
    role = "sr"
    scale = 2            # SR grid / LR grid: the operator-level backbones are built for the reference's x2 only

    def __init__(self, module: torch.nn.Module):
        super().__init__(module)
        self.record = os.environ.get("TPGSR_SR_RECORD", "1") != "0"

    # ---- recorded mode ------------------------------------------------------------------------------------------------------------
    def sr_plans(self, shape, training: bool, slot: int = 0) -> dict:
        key = (tuple(shape), bool(training), slot, K.POLICY)
        pl = self._plans.get(key)
        if pl is None:
            pl = self._plans[key] = self._trace_sr(tuple(shape), training)
        return pl

    def _trace_sr(self, shape, training):
        dev = self.device
        N = shape[0]
        lr = torch.empty(*shape, device=dev)
        prior = torch.empty(N, 37, 1, 26, device=dev)
        fwd = Plan("sr_tl_fwd")
        out = dict(fwd=fwd, lr=lr, prior=prior)
        with recording(fwd), K.conv_terms(K.terms_for("sr", "fwd")):
            if training:
                t = prior.requires_grad_(True)
                with torch.enable_grad():
                    y = self.module(lr, t)
            else:
                with torch.no_grad():
                    y = self.module(lr, prior)
        assert y.is_contiguous() and y.shape[0] == N
        out["sr"] = y.detach()
        if not training:
            return out
        bwd = Plan("sr_tl_bwd")
        bwd.overlap = os.environ.get("TPGSR_OVERLAP_WGRAD", "1") != "0"
        bwd.deferred = [] if os.environ.get("TPGSR_DEFER_REDUCE", "1") != "0" else None
        dsr = torch.empty_like(out["sr"])
        self.arena.attach_grads()
        grads = {p.data_ptr(): p.grad for p in self.module.parameters() if p.requires_grad}
        got = []
        h = t.register_hook(lambda g_: got.append(g_))
        prev, Fh.GRAD_SINK = Fh.GRAD_SINK, grads
        try:
            with recording(bwd), K.conv_terms(K.terms_for("sr", "bwd")):
                torch.autograd.backward(y, dsr)
                if bwd.deferred is not None:
                    K.flush_wgrad_reduces()
                K._REC.join()
        finally:
            Fh.GRAD_SINK = prev
            h.remove()
        t.grad = None
        if not got or not got[0].is_contiguous():
            raise RuntimeError(f"{type(self.module).__name__}: the traced backward pass produced no contiguous text-prior gradient")
        out.update(bwd=bwd, dsr=dsr, dprior=got[0], graph=y)       # `graph` keeps the saved activations alive
        return out

    # ---- the engine protocol --------------------------------------------------------------------------------------------------------
    def forward_pre(self, lr, training, slot: int = 0, defer_join: bool = False):
        """engine protocol: the prior-independent prologue `TSRNEngine` runs next to the text-prior generator.  Nothing here is worth
        splitting out (the first conv of these backbones is a fraction of a percent of the pass): a no-op"""
        return None

    def _check_mode(self, training):
        if bool(self.module.training) != bool(training):
            raise RuntimeError(f"{type(self.module).__name__}: forward(training={training}) on a module in "
                               f"{'train' if self.module.training else 'eval'}() mode")

    def forward(self, lr, training, prior=None, slot: int = 0, defer_join: bool = False, pre_done: bool = False) -> torch.Tensor:
        """lr (N, C, H, W), prior (N, 37, 1, 26) or None (zeros) -> SR image (N, C, 2H, 2W)"""
        self._check_mode(training)
        self.bind(lr.device)
        N = lr.shape[0]
        if prior is not None and tuple(prior.shape) != (N, 37, 1, 26):
            raise ValueError(f"{type(self.module).__name__}: the text prior is (N, 37, 1, 26), got {tuple(prior.shape)}")
        if self.record:
            pl = self.sr_plans(lr.shape, training, slot)
            K.copy(lr.contiguous(), pl["lr"], lr.numel())
            if prior is None:
                K.zero(pl["prior"], pl["prior"].numel())
            else:
                K.copy(prior.contiguous(), pl["prior"], prior.numel())
            pl["fwd"].run()
            if training:
                self._pending_batches += 1
                self._saved[slot] = (N, pl)
            res = torch.empty_like(pl["sr"])
            K.copy(pl["sr"], res, res.numel())
            return res
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
        if slot not in self._saved:
            raise RuntimeError(f"{type(self.module).__name__}: backward without a training-mode forward in slot {slot}")
        if self.record:
            n, pl = self._saved.pop(slot)
            assert n == x_shape[0]
            self.arena.attach_grads()                       # (same addresses as at trace time: the arena does not move)
            K.copy(dsr.contiguous(), pl["dsr"], pl["dsr"].numel())
            pl["bwd"].run()
            return pl["dprior"]        # the plan's buffer of this slot: valid until the slot's next backward pass
        t, y = self._saved.pop(slot)
        self.arena.attach_grads()
        with K.conv_terms(K.terms_for("sr", "bwd")):
            torch.autograd.backward(y, dsr.reshape(y.shape))
        return t.grad.contiguous()



class PlainSREngine(FunctionalSREngine):
    """`FunctionalSREngine` for a backbone WITHOUT a text prior: the reference's prior-free baselines (`--arch srres | rdn | vdsr`,
    model/{srresnet,rdn,vdsr}.py SRResNet / RDN / VDSR), which the `else:` branch of the train loop (interfaces/super_resolution.py:409-424)
    trains with `model(images_lr[:, :channel_num])`.  `SRTrainStep`, `FusedAdam`, `ArenaPool` and `TextSREvaluator` drive the module
    through this adapter; `module(x)` under autograd keeps working on its own.

    The same two modes: RECORDED (default, `TPGSR_SR_RECORD=0` switches it off) traces `module(lr)` once per (shape, training, slot,
    policy) into a forward and a backward plan -- parameter gradients through `functional.GRAD_SINK` into the arena, weight gradients on
    the weight-gradient stream with one batched slab reduce; otherwise operator by operator through autograd.  The input image needs no
    gradient, so the first layer's data gradient is never launched, and `backward` returns nothing."""

    def _trace_sr(self, shape, training):
        dev = self.device
        N = shape[0]
        lr = torch.empty(*shape, device=dev)
        fwd = Plan("sr_plain_fwd")
        out = dict(fwd=fwd, lr=lr)
        with recording(fwd), K.conv_terms(K.terms_for("sr", "fwd")):
            if training:
                with torch.enable_grad():
                    y = self.module(lr)
            else:
                with torch.no_grad():
                    y = self.module(lr)
        assert y.is_contiguous() and y.shape[0] == N
        out["sr"] = y.detach()
        if not training:
            return out
        bwd = Plan("sr_plain_bwd")
        bwd.overlap = os.environ.get("TPGSR_OVERLAP_WGRAD", "1") != "0"
        bwd.deferred = [] if os.environ.get("TPGSR_DEFER_REDUCE", "1") != "0" else None
        dsr = torch.empty_like(out["sr"])
        self.arena.attach_grads()
        grads = {p.data_ptr(): p.grad for p in self.module.parameters() if p.requires_grad}
        prev, Fh.GRAD_SINK = Fh.GRAD_SINK, grads
        try:
            with recording(bwd), K.conv_terms(K.terms_for("sr", "bwd")):
                torch.autograd.backward(y, dsr)
                if bwd.deferred is not None:
                    K.flush_wgrad_reduces()
                K._REC.join()
        finally:
            Fh.GRAD_SINK = prev
        out.update(bwd=bwd, dsr=dsr, graph=y)       # `graph` keeps the saved activations alive
        return out

    def forward(self, lr, training, prior=None, slot: int = 0, defer_join: bool = False, pre_done: bool = False) -> torch.Tensor:
        """lr (N, C, H, W) -> SR image (N, C, 2H, 2W)"""
        if prior is not None:
            raise ValueError(f"{type(self.module).__name__} takes no text prior")
        self._check_mode(training)
        self.bind(lr.device)
        if self.record:
            pl = self.sr_plans(lr.shape, training, slot)
            K.copy(lr.contiguous(), pl["lr"], lr.numel())
            pl["fwd"].run()
            if training:
                self._pending_batches += 1
                self._saved[slot] = (lr.shape[0], pl)
            res = torch.empty_like(pl["sr"])
            K.copy(pl["sr"], res, res.numel())
            return res
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
        if slot not in self._saved:
            raise RuntimeError(f"{type(self.module).__name__}: backward without a training-mode forward in slot {slot}")
        if self.record:
            n, pl = self._saved.pop(slot)
            assert n == x_shape[0]
            self.arena.attach_grads()                       # (same addresses as at trace time: the arena does not move)
            K.copy(dsr.contiguous(), pl["dsr"], pl["dsr"].numel())
            pl["bwd"].run()
            return None
        _, y = self._saved.pop(slot)
        self.arena.attach_grads()
        with K.conv_terms(K.terms_for("sr", "bwd")):
            torch.autograd.backward(y, dsr.reshape(y.shape))
        return None
