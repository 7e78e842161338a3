"""One layer of tpgsr_amd/engine_crnn.py at a time: the harness shared by tests/test_engine_crnn_layers_gpu.py and
tests/test_engine_crnn_layers_cpu.py.  Engine, launch log, policies, limits, generators and the error measure are those of
tests/engine_layer_common.py (imported, not restated).

Two run modes (`run_engine`), both ending with a synchronize:
  eager      OneLayerEngine.run: the layer's methods launch one by one; the weight gradients go out as single tpgsr_conv_wgrad launches, each
             followed by its tpgsr_wgrad_reduce
  recorded   the same fn recorded into a K.Plan with overlap = True and deferred = [], closed with K.flush_wgrad_reduces() and the
             recorder's join() (as CRNNEngine._record closes its backward plan), then plan.run(): under a split-operand policy the five
             weight gradients of a BiLSTM layer are tpgsr_conv_wgrad_batch launches, and every slab reduce is ONE tpgsr_wgrad_reduce_program
Every output and workspace buffer is pre-filled with NaN; every holder module ends with a `guard` parameter, and `arena_untouched` asserts
that the gradient arena is still zero everywhere outside the layer's own parameters (the guard, and the padding floats between tensors: the
37-class bias is followed by three of them).

The float64 references are stock PyTorch on the CPU with autograd and a seeded upstream gradient:
  BidirectionalLSTM  loader(x) -> torch.nn.LSTM(Cin, 256, bidirectional=True, batch_first=True) (functional_call, as
                     tests/test_functional_ops_gpu.py::_rnn_ref) -> F.linear                      (reference: model/crnn/crnn.py:5-26)
  behind BatchNorm   F.batch_norm(training=True) -> ReLU -> the same                              (reference: model/crnn/crnn.py:52-55, 69-72)
  conv0              F.conv2d(gray, w, b, padding=1)                                              (reference: model/crnn/crnn.py:45-46)
`model_terms` is the error model of the fewer-term policies: the same computation in float64 with the operands of every GEMM the engine runs
on the split-bf16 convolution kernels rounded to the policy's number of bf16 terms (x2: two, bf16: one), as
tests/test_gru_proj_gpu.py::matrix_reference builds its one-term model; the recurrent products stay exact (csrc/lstm_seq.hip multiplies
three-term operands under every policy)."""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from engine_layer_common import (F64, FLOOR, POLICIES, TERMS, OneLayerEngine, T, _gen, _pack_names, arith_bound, conv_prec, err,  # noqa: E402,F401
                                 launch_log, limits)

HH = 256                 # the persistent kernels take nothing else, and the reference builds nothing else
G4 = 4 * HH
MODES = ("eager", "recorded")
LSTM_KEYS = tuple("rnn." + k for k in T._RNN_KEYS) + ("embedding.weight", "embedding.bias")
MODEL_MARGIN = 4         # the suite's usual factor over a reference-derived error


def _dev(device):
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def run_engine(eng, fn, device, mode):
    """fn(engine, layer) under the run mode; -> the workspace the slab buffers of a recorded run live in (None when eager)"""
    assert mode in MODES
    if mode == "eager":
        eng.run(fn, device)
        return None
    from tpgsr_amd import engine, kernels as K
    device = _dev(device)
    eng.bind(device)
    eng.arena.grad.zero_()
    ws = eng._cur_ws = engine._Ws(device)
    eng._wg_idx = 0
    plan = K.Plan("one_layer_recorded")
    plan.overlap, plan.deferred = True, []
    with K.recording(plan):
        eng.pack_all()
        fn(eng, eng.layer)
        eng.flush_compose_bwd()
        K.flush_wgrad_reduces()
        K._REC.join()
    for t in ws.t.values():                              # the slab buffers of the deferred reduces
        if isinstance(t, torch.Tensor) and t.is_floating_point():
            t.fill_(float("nan"))
    plan.run()
    if not K.DRYRUN:
        torch.cuda.synchronize()
    eng._plan = plan
    return ws


def arena_untouched(eng, names):
    """the gradient arena is zero outside the parameters `names`: the guard's gradient and every padding float between two tensors"""
    o = eng.arena.offsets
    assert GUARD in o and o[GUARD] == max(o.values()), "the guard is the last tensor of the arena"
    g = eng.arena.grad.detach().cpu().clone()
    for n in names:
        g[o[n]:o[n] + eng.P[n].numel()] = 0
    assert not bool(torch.isnan(g).any()) and not bool(g.any()), \
        f"a gradient was written outside the layer's parameters, at arena offsets {g.nonzero().flatten()[:8].tolist()} (the guard starts at {o[GUARD]})"


GUARD = "end.guard"


class _Guard(torch.nn.Module):
    """the holder's LAST child (a module's own parameters come before its children's in named_parameters(), which is the arena's order)"""

    def __init__(self, n):
        super().__init__()
        self.guard = torch.nn.Parameter(torch.zeros(n))


def _fill(module, params, prefix):
    with torch.no_grad():
        have = dict(module.named_parameters())
        want = {prefix + k for k in params}
        assert want <= set(have) and set(have) - want <= {GUARD}, sorted(have)
        for k, v in params.items():
            assert have[prefix + k].shape == v.shape, (k, tuple(have[prefix + k].shape), tuple(v.shape))
            have[prefix + k].copy_(v)


# ---- LstmLayer -----------------------------------------------------------------------------------------------------------
LSTM_LAYERS = [  # name, Cin, nOut, loader
    ("rnn0", 512, 256, "relu"),        # in_scale, in_shift, in_act="relu" (behind bn6 + ReLU); embedding: ConvLayer
    ("rnn1", 256, 37, "none"),         # embedding: PaddedLinear, Cp = 40
]
LSTM_MAPS = [(2, 5), (3, 26), (1, 33), (64, 2)]          # ragged everything; the CRNN's T, odd batch; T > 31: counter hand-off; the batch limit


def _lstm_params(g, Cin, nOut):
    rnn = T._rnn_params(g, Cin, HH, 4)
    p = {"rnn." + k: rnn[n] for k, n in zip(T._RNN_KEYS, T._GRU_NAMES)}
    b = 1.0 / (2 * HH) ** 0.5
    p["embedding.weight"] = (torch.rand(nOut, 2 * HH, generator=g) * 2 - 1) * b
    p["embedding.bias"] = (torch.rand(nOut, generator=g) * 2 - 1) * b
    return p


def _bf_terms(x, k):
    """x rounded to the sum of k bf16 terms (round to nearest even each: the operand split of csrc/conv_xbf.hip)"""
    s = torch.zeros_like(x)
    for _ in range(k):
        s = s + (x - s).to(torch.float32).to(torch.bfloat16).to(x.dtype)
    return s


class _RoundedMM(torch.autograd.Function):
    """y = r(a) r(w)^T, da = r(dy) r(w), dw = r(dy)^T r(a): the three GEMMs of a layer, each on operands rounded to k bf16 terms"""

    @staticmethod
    def forward(ctx, a, w, k):
        ctx.save_for_backward(a, w)
        ctx.k = k
        return _bf_terms(a, k) @ _bf_terms(w, k).T

    @staticmethod
    def backward(ctx, dy):
        a, w = ctx.saved_tensors
        k = ctx.k
        dyr = _bf_terms(dy, k)
        return dyr @ _bf_terms(w, k), dyr.T @ _bf_terms(a, k), None


def _mm(a, w, k):
    return a @ w.T if k == 0 else _RoundedMM.apply(a, w, k)


def _lstm_manual(a, p, k):
    """nn.LSTM's equations (gate order i, f, g, o), bidirectional, in a's dtype; the input projection's and the hidden-side weight
    gradient's GEMMs on k-term operands (k = 0: exact), the recurrent product h W_hh^T and its data gradient exact.
    a [N][T][Cin] -> out [N][T][2 Hh]"""
    N, T_, _ = a.shape
    outs = []
    for d, suf in enumerate(("", "_reverse")):
        wih, whh = p["rnn.weight_ih_l0" + suf], p["rnn.weight_hh_l0" + suf]
        gi = _mm(a.reshape(N * T_, -1), wih, k).reshape(N, T_, G4) + p["rnn.bias_ih_l0" + suf] + p["rnn.bias_hh_l0" + suf]
        h, c = a.new_zeros(N, HH), a.new_zeros(N, HH)
        hs = [None] * T_
        for t in (range(T_) if d == 0 else range(T_ - 1, -1, -1)):
            if k == 0:
                gh = h @ whh.T
            else:   # value and dh through the exact product, dW_hh through the k-term one (the engine's tpgsr_conv_wgrad over out and dG)
                gh = h @ whh.detach().T + (_mm(h.detach(), whh, k) - _mm(h.detach(), whh.detach(), k))
            q = gi[:, t] + gh
            i_, f_, g_, o_ = torch.sigmoid(q[:, :HH]), torch.sigmoid(q[:, HH:2 * HH]), torch.tanh(q[:, 2 * HH:3 * HH]), torch.sigmoid(q[:, 3 * HH:])
            c = f_ * c + i_ * g_
            h = o_ * torch.tanh(c)
            hs[t] = h
        outs.append(torch.stack(hs, 1))
    return torch.cat(outs, -1)


def persistent(device):
    """do the layers record the persistent recurrences on `device`?  Whatever K.lstm_seq_coresident answers, exactly as the engine asks"""
    from tpgsr_amd import kernels as K
    return bool(K.LSTM_SEQ and K.LSTM_SEQ_BWD and K.lstm_seq_coresident(_dev(device)))


def _recurrence_names(T_, per_step, granule):
    """(forward, backward) launches of the recurrence: one persistent launch each, or tpgsr_lstm_rec_gemm (from step 1 on) + the gate kernel per step"""
    if per_step:
        return ([n for s in range(T_) for n in (["tpgsr_lstm_rec_gemm"] if s else []) + ["tpgsr_lstm_step_fwd"]],
                [n for s in range(T_) for n in (["tpgsr_lstm_rec_gemm"] if s else []) + ["tpgsr_lstm_step_bwd"]])
    return ["tpgsr_lstm_seq_fwdg" if (granule and T_ <= 31) else "tpgsr_lstm_seq_fwd"], ["tpgsr_lstm_seq_bwd"]


class LstmCase:
    def __init__(self, name, Cin, nOut, loader, N, T_):
        self.name, self.Cin, self.nOut, self.loader, self.N, self.T = name, Cin, nOut, loader, N, T_
        self.id = f"{name}-{N}x{T_}"
        self.M = M = N * T_
        self.padded = nOut % 4 != 0
        self.Cp = (nOut + 3) // 4 * 4
        g = _gen("engine-lstm", self.id)
        self.params = _lstm_params(g, Cin, nOut)
        ins = {}
        if loader == "relu":     # the post-affine value z is drawn, pushed away from the ReLU's kink, and x = (z - shift) / scale
            ins["scale"], ins["shift"] = torch.rand(Cin, generator=g) + 0.5, torch.randn(Cin, generator=g)
            z = T._away(torch.randn(M, Cin, generator=g))
            ins["x"] = ((z.double() - ins["shift"].double()) / ins["scale"].double()).float()
        else:
            ins["x"] = torch.randn(M, Cin, generator=g)
        self.ins = ins
        self.de = torch.randn(M, nOut, generator=_gen("engine-lstm-upstream", self.id))
        self._ref, self._model = None, {}

    def loader_kwargs(self, d):
        return dict(in_scale=d["scale"], in_shift=d["shift"], in_act="relu") if self.loader == "relu" else {}

    def pre_activation(self, dtype=F64):
        """z = x * scale + shift of the float32-rounded inputs (None without a loader)"""
        if self.loader != "relu":
            return None
        d = {k: v.to(dtype) for k, v in self.ins.items()}
        return d["x"] * d["scale"] + d["shift"]

    def loader_out(self, dtype):
        z = self.pre_activation(dtype)
        return self.ins["x"].to(dtype) if z is None else torch.relu(z)

    def _autograd(self, dtype, k=None):
        """{e, out, dx, every parameter gradient}; k None: torch.nn.LSTM + F.linear; k >= 0: the manual recurrence with k-term GEMM operands"""
        N, T_, M = self.N, self.T, self.M
        a = self.loader_out(dtype).clone().requires_grad_(True)
        p = {n: v.to(dtype).clone().requires_grad_(True) for n, v in self.params.items()}
        if k is None:
            d = {n: p["rnn." + key] for key, n in zip(T._RNN_KEYS, T._GRU_NAMES)}
            out = T._rnn_ref(torch.nn.LSTM, a.view(N, T_, self.Cin), d, HH).reshape(M, 2 * HH)
            e = F.linear(out, p["embedding.weight"], p["embedding.bias"])
        else:
            out = _lstm_manual(a.view(N, T_, self.Cin), p, k).reshape(M, 2 * HH)
            e = _mm(out, p["embedding.weight"], k) + p["embedding.bias"]
        e.backward(self.de.to(dtype))
        res = {"e": e.detach(), "out": out.detach(), "dx": a.grad}
        res.update({n: p[n].grad for n in LSTM_KEYS})
        return res

    def reference(self):
        """float64, torch.nn.LSTM: computed once and never modified"""
        if self._ref is None:
            self._ref = self._autograd(F64)
        return self._ref

    def model_terms(self, policy):
        """per key: MODEL_MARGIN x e(the float64 computation on k-term GEMM operands, the float64 reference); {} under x3 / f32.
        From the reference alone -- nothing the GPU computed enters it."""
        k = TERMS[policy]
        if k not in (1, 2):
            return {}
        if k not in self._model:
            ref = self.reference()
            exact = self._autograd(F64, 0)              # the manual recurrence itself agrees with torch.nn.LSTM to float64 rounding
            assert all(err(exact[n], ref[n]) < 1e-12 for n in ref), {n: err(exact[n], ref[n]) for n in ref}
            rounded = self._autograd(F64, k)
            self._model[k] = {n: MODEL_MARGIN * err(rounded[n], ref[n]) for n in ref}
        return self._model[k]

    # -- what the engine is expected to launch (LstmLayer's code) --
    def expected_launches(self, policy, mode="eager", passes=1, per_step=False, granule=True):
        T_ = self.T
        split = bool(TERMS[policy])
        rec = mode == "recorded"
        batch = split and rec                                        # K.LSTM_WGRAD_BATCH and K.CONV_TERMS > 0 and K.deferring()
        reduce1 = [] if rec else ["tpgsr_wgrad_reduce"]              # recorded: deferred to the one reduce program at the end
        fseq, bseq = _recurrence_names(T_, per_step, granule)
        fwd = ["tpgsr_conv_fwd"] + fseq + ["tpgsr_conv_fwd"]         # input projection, recurrence, embedding
        bwd = ["tpgsr_pad_channels"] if self.padded else []          # dlogits padded to Cp classes, as CRNNEngine._record_bwd does
        if not batch:
            bwd += ["tpgsr_conv_wgrad"] + reduce1                    # the embedding's own wgrad()
        bwd += ["tpgsr_conv_fwd"] + bseq                             # d out, BPTT
        if batch:
            # tpgsr_conv_wgrad_batch takes launches of ONE loader variant: rnn0's two input-side GEMMs read x through the BatchNorm +
            # ReLU loader (variant 3), the embedding and the two hidden-side ones are plain (variant 0) -> a batch of three and a second
            # batch launch of two; rnn1 has no loader -> one batch of five
            bwd += ["tpgsr_conv_wgrad_batch"] * (2 if self.loader == "relu" else 1)
        else:
            bwd += (["tpgsr_conv_wgrad"] + reduce1) * 4
        bwd += ["tpgsr_conv_fwd"]                                    # dx
        return _pack_names(policy) + (fwd + bwd) * passes + (["tpgsr_wgrad_reduce_program"] if rec else [])


def lstm_cases():
    return [LstmCase(*L, *m) for L in LSTM_LAYERS for m in LSTM_MAPS]


# what tests/test_engine_crnn_layers_gpu.py runs besides every case x every policy, eagerly (the CPU file records exactly these)
RECORDED = [(f"{n}-{m}", p) for n in ("rnn0", "rnn1") for m in ("2x5", "3x26") for p in ("x3", "x2")]
PER_STEP = [(cid, p) for cid in ("rnn0-2x5", "rnn1-2x5") for p in ("x3", "f32")]           # K.LSTM_SEQ / K.LSTM_SEQ_BWD off: ten small launches
GRANULE_OFF = [("rnn0-2x5", "x3"), ("rnn1-3x26", "x3")]                                    # K.LSTM_GRANULE off
TWO_PASSES = [("rnn0-2x5", "x3"), ("rnn1-3x26", "x2")]
BN_POLICIES = ("x3", "f32")


def lstm_holder(case, bn=False):
    """the project's BidirectionalLSTM under the prefix `l` (behind `bn`: BatchNormParams, when asked), then the guard"""
    from tpgsr_amd.model import nn_params
    from tpgsr_amd.model.crnn import crnn

    class Holder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            if bn:
                self.bn = nn_params.BatchNormParams(case.Cin)
            self.l = crnn.BidirectionalLSTM(case.Cin, HH, case.nOut)
            self.end = _Guard(4 * 2 * HH)
    m = Holder()
    params = {"l." + k: v for k, v in case.params.items()}
    if bn:
        params.update({"bn.weight": case.gamma, "bn.bias": case.beta})
    _fill(m, params, "")
    return m


def _nan(device, *s):
    return torch.full(s, float("nan"), device=device)


def lstm_buffers(case, device):
    N, T_, M = case.N, case.T, case.M
    return dict(G=_nan(device, M, 2 * G4), gh=_nan(device, HH // 32, 2, N, G4), Cst=_nan(device, M, 2 * HH), out=_nan(device, M, 2 * HH),
                e=_nan(device, M, case.nOut), dout=_nan(device, M, 2 * HH), dhc=_nan(device, G4 // 32, 2, N, HH), dcc=_nan(device, N, 2 * HH),
                dx=_nan(device, M, case.Cin), de_p=_nan(device, M, case.Cp))


def seq_timeouts(L):
    """the hand-off time-out word (sync[2]) of every exchange buffer the layer's persistent launches used"""
    words = []
    for name in ("_seq", "_seqb"):
        for key, (_buf, sync) in getattr(L, name, {}).items():
            words.append((name, int(sync.cpu()[2])))
    return words


def run_lstm(case, device, mode="eager", passes=1):
    """the engine's LstmLayer on the case: ({e, out, dx, parameter gradients} on the CPU, the launches, the engine).
    passes: forward + backward that many times on one gradient arena (the backward pass overwrites the saved gates with their gradients)"""
    from tpgsr_amd import engine_crnn, kernels as K
    eng = OneLayerEngine(lstm_holder(case), lambda e: engine_crnn.LstmLayer(e, "l"))
    d = {k: v.to(device).contiguous() for k, v in case.ins.items()}
    kw = case.loader_kwargs(d)
    buf = lstm_buffers(case, device)
    de = case.de.to(device).contiguous()
    N, T_ = case.N, case.T

    def fn(eng, L):
        assert isinstance(L.emb, engine_crnn.PaddedLinear) == case.padded and L.emb.Cout == case.nOut
        for _ in range(passes):
            L.fwd(N, T_, d["x"], buf["G"], buf["gh"], buf["Cst"], buf["out"], buf["e"], **kw)
            de_in = de
            if case.padded:
                assert L.emb.Cp == case.Cp
                K.pad_channels(de, case.M, case.nOut, case.Cp, buf["de_p"])
                de_in = buf["de_p"]
            L.bwd(N, T_, d["x"], buf["G"], buf["Cst"], buf["out"], de_in, buf["dout"], buf["dhc"], buf["dcc"], buf["dx"], **kw)

    with launch_log() as names:
        run_engine(eng, fn, device, mode)
    got = {"e": buf["e"].cpu(), "out": buf["out"].cpu(), "dx": buf["dx"].cpu()}
    for k, v in case.params.items():
        got[k] = eng.G["l." + k].cpu().view(v.shape)
    if not K.DRYRUN:
        assert all(w == 0 for _n, w in seq_timeouts(eng.layer)), seq_timeouts(eng.layer)
    arena_untouched(eng, ["l." + k for k in case.params])
    return got, names, eng


# ---- the first BiLSTM behind a real BatchNorm ------------------------------------------------------------------------------
BN_SEEDS = tuple(range(201, 233))
BN_MAPS = [(2, 5), (3, 26)]          # M = 10 rows; M = 78: two 64-row blocks, the second ragged
BN_KEYS = ("bn.weight", "bn.bias")
BN_EPS = 1e-5
BN_MARGIN_FACTOR = 64


class BnLstmCase(LstmCase):
    """BatchNorm2d(512), training mode -> ReLU -> BidirectionalLSTM(512, 256, 256).  s [M][512] is the pre-BatchNorm tensor: the first seed
    of BN_SEEDS whose float64 min |bn(s)| exceeds 64 x the max absolute error of the float32 bn(s) on the CPU (nothing is masked)"""

    def __init__(self, N, T_):
        super().__init__("bn+rnn0", 512, 256, "none", N, T_)
        g = _gen("engine-bn-lstm", self.id)
        self.gamma, self.beta = torch.rand(512, generator=g) + 0.5, torch.randn(512, generator=g) * 0.5
        self.seed = self.margin = self.noise = None
        for seed in BN_SEEDS:
            s = torch.randn(self.M, 512, generator=_gen("engine-bn-lstm-s", self.id, seed)) * 1.5 + 0.25
            z64, z32 = self._bn(s, F64), self._bn(s, torch.float32)
            margin, noise = z64.abs().min().item(), (z32.double() - z64).abs().max().item()
            if margin > BN_MARGIN_FACTOR * noise:
                self.seed, self.margin, self.noise = seed, margin, noise
                break
        assert self.seed is not None, "no seed of BN_SEEDS keeps bn(s) clear of the ReLU's kink"
        self.ins = {"x": s}

    def _bn(self, s, dtype, gamma=None, beta=None):
        gamma = self.gamma.to(dtype) if gamma is None else gamma
        beta = self.beta.to(dtype) if beta is None else beta
        return F.batch_norm(s.to(dtype), None, None, gamma, beta, training=True, eps=BN_EPS)

    def _autograd(self, dtype, k=None):
        N, T_, M = self.N, self.T, self.M
        s = self.ins["x"].to(dtype).clone().requires_grad_(True)
        gamma, beta = self.gamma.to(dtype).clone().requires_grad_(True), self.beta.to(dtype).clone().requires_grad_(True)
        a = torch.relu(self._bn(s, dtype, gamma, beta))
        p = {n: v.to(dtype).clone().requires_grad_(True) for n, v in self.params.items()}
        if k is None:
            d = {n: p["rnn." + key] for key, n in zip(T._RNN_KEYS, T._GRU_NAMES)}
            out = T._rnn_ref(torch.nn.LSTM, a.view(N, T_, self.Cin), d, HH).reshape(M, 2 * HH)
            e = F.linear(out, p["embedding.weight"], p["embedding.bias"])
        else:
            out = _lstm_manual(a.view(N, T_, self.Cin), p, k).reshape(M, 2 * HH)
            e = _mm(out, p["embedding.weight"], k) + p["embedding.bias"]
        e.backward(self.de.to(dtype))
        res = {"e": e.detach(), "out": out.detach(), "ds": s.grad, "bn.weight": gamma.grad, "bn.bias": beta.grad}
        res.update({n: p[n].grad for n in LSTM_KEYS})
        return res

    def expected_launches(self, policy, per_step=False):
        fused = bool(TERMS[policy])          # K.bnb_fusable(2 * G4): the epilogue rides on the split-bf16 kernels only
        fseq, bseq = _recurrence_names(self.T, per_step, True)
        names = _pack_names(policy) + ["tpgsr_bn_stats", "tpgsr_bn_finalize"]
        names += ["tpgsr_conv_fwd"] + fseq + ["tpgsr_conv_fwd"]
        names += ["tpgsr_conv_wgrad", "tpgsr_wgrad_reduce", "tpgsr_conv_fwd"] + bseq + ["tpgsr_conv_wgrad", "tpgsr_wgrad_reduce"] * 4
        names += ["tpgsr_conv_fwd"] + ([] if fused else ["tpgsr_bn_bwd_reduce"]) + ["tpgsr_bn_bwd_finalize", "tpgsr_bn_bwd_apply"]
        return names


def bn_cases():
    return [BnLstmCase(*m) for m in BN_MAPS]


def run_bn_lstm(case, device):
    """training-mode BatchNorm finalize, the loader from bn.loader, fz = bn.fuse_stats(...), L.bwd(..., dx_bnb=fz), bn.backward(..., fused=fz):
    ({e, out, ds, every parameter gradient} on the CPU, the launches, whether the epilogue was fused)"""
    from tpgsr_amd import engine, engine_crnn, kernels as K
    # (.to: the running statistics are buffers, which the engine wants on the parameters' device)
    eng = OneLayerEngine(lstm_holder(case, bn=True).to(device), lambda e: (engine.BNLayer(e, "bn"), engine_crnn.LstmLayer(e, "l")))
    s = case.ins["x"].to(device).contiguous()
    buf = lstm_buffers(case, device)
    ds = _nan(device, case.M, case.Cin)
    de = case.de.to(device).contiguous()
    N, T_, M = case.N, case.T, case.M
    seen = {}

    def fn(eng, layers):
        bn, L = layers
        bn.use(eng._cur_ws)
        for t in eng._cur_ws.t[("bn", "bn")][2:]:
            t.fill_(float("nan"))                       # save_mean, save_rstd, coef
        part, nblk = bn.partial(M)
        part.fill_(float("nan"))
        K.bn_stats(s, M, bn.C, part, nblk)
        bn.finalize(M, None, True)
        kw = dict(in_act="relu", **bn.loader)
        L.fwd(N, T_, s, buf["G"], buf["gh"], buf["Cst"], buf["out"], buf["e"], **kw)
        fz = bn.fuse_stats(s, M, "relu", 2 * G4)
        if fz is not None:
            fz["partial"].fill_(float("nan"))
        seen["fused"] = fz is not None
        L.bwd(N, T_, s, buf["G"], buf["Cst"], buf["out"], de, buf["dout"], buf["dhc"], buf["dcc"], buf["dx"], dx_bnb=fz, **kw)
        bn.backward(buf["dx"], None, s, M, "relu", ds, fused=fz)

    with launch_log() as names:
        eng.run(fn, device)
    got = {"e": buf["e"].cpu(), "out": buf["out"].cpu(), "ds": ds.cpu()}
    for k, v in case.params.items():
        got[k] = eng.G["l." + k].cpu().view(v.shape)
    for k in BN_KEYS:
        got[k] = eng.G[k].cpu().clone()
    if not K.DRYRUN:
        assert all(w == 0 for _n, w in seq_timeouts(eng.layer[1])), seq_timeouts(eng.layer[1])
    arena_untouched(eng, ["l." + k for k in case.params] + list(BN_KEYS))
    return got, names, seen["fused"]


# ---- Conv0Im2col ---------------------------------------------------------------------------------------------------------
CONV0_MAPS = [(1, 5, 7), (2, 32, 100), (3, 3, 257)]


class Conv0Case:
    """Conv2d(1, 64, 3, 1, 1) on gray [N][1][H][W]"""

    def __init__(self, N, H, W):
        self.N, self.H, self.W = N, H, W
        self.id = f"conv0-{N}x{H}x{W}"
        g = _gen("engine-conv0", self.id)
        self.params = {"weight": (torch.rand(64, 1, 3, 3, generator=g) * 2 - 1) / 3, "bias": (torch.rand(64, generator=g) * 2 - 1) / 3}
        self.gray = torch.randn(N, 1, H, W, generator=g)
        self.dy = torch.randn(N * H * W, 64, generator=g)
        self._ref, self._model = None, {}

    def _autograd(self, dtype, k=0):
        N, H, W = self.N, self.H, self.W
        x = self.gray.to(dtype).clone().requires_grad_(True)
        w, b = (self.params[n].to(dtype).clone().requires_grad_(True) for n in ("weight", "bias"))
        if k == 0:
            y = F.conv2d(x, w, b, padding=1)
        else:          # the engine's form: im2col (exact), then the three GEMMs on k-term operands, col2im (exact)
            col = F.unfold(x, 3, padding=1).transpose(1, 2).reshape(N * H * W, 9)
            y = (_mm(col, w.view(64, 9), k) + b).view(N, H, W, 64).permute(0, 3, 1, 2)
        y.backward(self.dy.to(dtype).view(N, H, W, 64).permute(0, 3, 1, 2))
        return {"y": y.detach().permute(0, 2, 3, 1).reshape(N * H * W, 64), "dw": w.grad, "db": b.grad, "dgray": x.grad}

    def reference(self):
        if self._ref is None:
            self._ref = self._autograd(F64)
        return self._ref

    def model_terms(self, policy):
        k = TERMS[policy]
        if k not in (1, 2):
            return {}
        if k not in self._model:
            ref, rounded = self.reference(), self._autograd(F64, k)
            self._model[k] = {n: MODEL_MARGIN * err(rounded[n], ref[n]) for n in ref}
        return self._model[k]

    def expected_launches(self, policy):
        return _pack_names(policy) + ["tpgsr_im2col3x3_c1", "tpgsr_conv_fwd", "tpgsr_conv_wgrad", "tpgsr_wgrad_reduce_program", "tpgsr_conv_fwd",
                                      "tpgsr_col2im3x3_c1"]


def conv0_cases():
    return [Conv0Case(*m) for m in CONV0_MAPS]


def conv0_holder(case):
    from tpgsr_amd.model import nn_params

    class Holder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.c = nn_params.Conv2dParams(1, 64, 3, padding=1)
            self.end = _Guard(4 * 64)
    m = Holder()
    _fill(m, {"c." + k: v for k, v in case.params.items()}, "")
    return m


def run_conv0(case, device):
    from tpgsr_amd import engine_crnn
    eng = OneLayerEngine(conv0_holder(case), lambda e: engine_crnn.Conv0Im2col(e, "c.weight", "c.bias"))
    N, H, W = case.N, case.H, case.W
    P = N * H * W
    gray, dy = case.gray.to(device).contiguous(), case.dy.to(device).contiguous()
    col, y, dcol, dgray = _nan(device, P, 12), _nan(device, P, 64), _nan(device, P, 12), _nan(device, N, 1, H, W)

    def fn(eng, L):
        L.fwd(N, H, W, gray, col, y)
        L.wgrad(N, H, W, col, dy)
        L.dgrad(N, H, W, dy, dcol, dgray)

    with launch_log() as names:
        eng.run(fn, device)
    arena_untouched(eng, ["c.weight", "c.bias"])
    return {"y": y.cpu(), "dw": eng.G["c.weight"].cpu().view(64, 1, 3, 3), "db": eng.G["c.bias"].cpu().clone(), "dgray": dgray.cpu()}, names


# ---- tpgsr_im2col3x3_c1 / tpgsr_col2im3x3_c1 / tpgsr_pad_channels, called directly ---------------------------------------------
COL_SHAPES = [(1, 1, 1), (2, 3, 5), (3, 32, 100), (1, 7, 257)]
PAD_SHAPES = [(1, 37, 40), (130, 37, 40), (7, 3, 3), (1000, 5, 8)]      # (M, Cs, Cd)


def im2col_case(N, H, W):
    """gray and what F.unfold makes of it: [N H W][9] float32 (a gather: exact)"""
    gray = torch.randn(N, 1, H, W, generator=_gen("im2col", N, H, W))
    return gray, F.unfold(gray, 3, padding=1).transpose(1, 2).reshape(N * H * W, 9).contiguous()


def col2im_case(N, H, W):
    """dcol [N H W][12] with NON-ZERO garbage in columns 9..11, and the float64 / float32 adjoint of im2col over columns 0..8"""
    P = N * H * W
    dcol = torch.randn(P, 12, generator=_gen("col2im", N, H, W))
    dcol[:, 9:] = dcol[:, 9:] * 100 + 1000

    def ref(dtype):
        x = torch.zeros(N, 1, H, W, dtype=dtype, requires_grad=True)
        col = F.unfold(x, 3, padding=1).transpose(1, 2).reshape(P, 9)
        col.backward(dcol[:, :9].to(dtype))
        return x.grad
    return dcol, ref(F64), ref(torch.float32)


def pad_case(M, Cs, Cd):
    src = torch.randn(M, Cs, generator=_gen("pad-channels", M, Cs, Cd))
    return src, torch.cat([src, torch.zeros(M, Cd - Cs)], 1)
