"""One layer of tpgsr_amd/engine.py at a time: the harness shared by tests/test_engine_gru_layer_gpu.py, tests/test_engine_strip_fold_gpu.py
and tests/test_engine_layers_cpu.py.

`OneLayerEngine(module, build)` is an `engine._EngineBase` whose `_build_layers` makes ONE layer object (GruLayer, TConvStrip, FoldedDgrad)
over the parameters of a small holder module.  `run(fn)` binds, zeroes the gradient arena, packs the operands (pack program + bf16 split,
as a training forward does), calls the layer's own methods eagerly -- no plan recorder -- and ends with `flush_compose_bwd()`: what runs is
the engine's code (operand layouts, branch choice, slab reduces, chain rule), not a copy of its launch sequence.  `launch_log()` lists the
C-ABI entry points that were launched, so every test can assert which branch it covered; `expected_launches` is that branch table written
down from the layer classes' docstrings, as a function of the case alone.

The float64 references are stock PyTorch on the CPU with autograd and a seeded upstream gradient:
  GruBlock   loader -> F.conv2d 1x1 -> torch.nn.GRU(U, Hd, bidirectional=True, batch_first=True) along the axis (functional_call, as
             tests/test_functional_ops_gpu.py::_rnn_ref)                                         (reference: model/tsrn.py:491-508)
  TConvStrip F.conv_transpose2d on the H = 1 strip                                               (InfoGen, model/tsrn.py:81-108)
  FoldedDgrad  the input gradient of F.conv2d(x, w, padding=KS // 2)                             (block1, model/tsrn.py:28)
`_gen`, `err`, `FLOOR`, `F64` and `CONV_LIMITS` are those of tests/test_functional_ops_gpu.py (imported, not restated)."""
import contextlib
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_functional_ops_gpu as T  # noqa: E402
from test_functional_ops_gpu import CONV_LIMITS, F64, FLOOR, _gen, err  # noqa: E402,F401  (re-exported)

POLICIES = ("x3", "x2", "bf16", "f32")
TERMS = {"x3": 3, "x2": 2, "bf16": 1, "f32": 0}
BF16_LIMIT = 2e-2        # every terms = 1 kernel test of the suite (test_conv_panel_gpu, test_conv_halo3_gpu, test_wgrad3_gpu)


def limits(policy):
    """(values and data gradients, parameter gradients)"""
    if policy == "bf16":
        return BF16_LIMIT, BF16_LIMIT
    return CONV_LIMITS["x3" if policy == "f32" else policy]


# ---- the engine ----------------------------------------------------------------------------------------------------------
def _engine_base():
    from tpgsr_amd import engine
    return engine


def OneLayerEngine(module, build):
    """an engine._EngineBase over `module` whose only layer is build(engine)   (the package is imported here, not with this module)"""
    from tpgsr_amd import engine, kernels as K

    class _OneLayerEngine(engine._EngineBase):
        def _build_layers(self):
            self.layer = build(self)

        def run(self, fn, device):
            """fn(engine, layer): the launches of one forward + backward pass of the layer, eagerly"""
            device = torch.device(device)
            if device.type == "cuda" and device.index is None:
                device = torch.device("cuda", torch.cuda.current_device())
            self.bind(device)
            self.arena.grad.zero_()
            self._cur_ws = engine._Ws(device)
            self.pack_all()
            fn(self, self.layer)
            self.flush_compose_bwd()
            if not K.DRYRUN:
                torch.cuda.synchronize()
    return _OneLayerEngine(module)


@contextlib.contextmanager
def launch_log():
    """names of the C-ABI entry points launched (or recorded) inside, in order"""
    from tpgsr_amd import kernels as K
    names, inner = [], K._launch

    def logged(name, *args):
        names.append(name)
        return inner(name, *args)
    K._launch = logged
    try:
        yield names
    finally:
        K._launch = inner


@contextlib.contextmanager
def conv_prec(policy):
    from tpgsr_amd import kernels as K
    prev = K.POLICY
    K.set_conv_prec(policy)
    try:
        yield
    finally:
        K.set_conv_prec(prev)


def _pack_names(policy):
    return ["tpgsr_pack_program"] + (["tpgsr_split_bf_program"] if TERMS[policy] else [])


# ---- GruLayer ------------------------------------------------------------------------------------------------------------
GRU_LAYERS = [  # Cin, U, Hd, axis, loader
    (64, 64, 32, 0, "residual"),           # gru2 of TSRN
    (64, 64, 32, 1, "affine"),             # gru1 of TSRN
    (96, 64, 32, 1, "affine+strip"),       # gru1 of TSRN_TL
    (128, 128, 64, 0, "residual"),         # the same three at hidden_units = 64
    (128, 128, 64, 1, "affine"),
    (160, 128, 64, 1, "affine+strip"),
]
GRU_MAPS = [(2, 16, 64), (1, 16, 64), (2, 5, 7)]
GRU_KEYS = ("conv1.weight", "conv1.bias") + tuple("gru." + k for k in T._RNN_KEYS)
STRIP = 32      # channels of the text strip


class GruCase:
    def __init__(self, Cin, U, Hd, axis, loader, N, H, W):
        self.Cin, self.U, self.Hd, self.axis, self.loader, self.N, self.H, self.W = Cin, U, Hd, axis, loader, N, H, W
        self.id = f"C{Cin}-U{U}-axis{axis}-{loader}-{N}x{H}x{W}"
        self.P = P = N * H * W
        g = _gen("engine-gru", self.id)
        ca = Cin - STRIP if loader == "affine+strip" else Cin
        ins = {"x": torch.randn(P, ca, generator=g)}
        if loader in ("affine", "affine+strip"):
            ins["scale"], ins["shift"] = torch.rand(Cin, generator=g) + 0.5, torch.randn(Cin, generator=g)
        if loader == "affine+strip":
            ins["scale"][ca:], ins["shift"][ca:] = 1.0, 0.0            # (engine.BNLayer pads its scale / shift with the identity)
            ins["strip"] = torch.randn(N * W, STRIP, generator=g)
        if loader == "residual":
            ins["x2"] = torch.randn(P, Cin, generator=g)
        self.ins, self.cin_a = ins, ca
        b = 1.0 / Cin ** 0.5
        rnn = T._rnn_params(g, U, Hd, 3)
        self.params = {"conv1.weight": (torch.rand(U, Cin, 1, 1, generator=g) * 2 - 1) * b, "conv1.bias": (torch.rand(U, generator=g) * 2 - 1) * b}
        self.params.update({"gru." + k: rnn[n] for k, n in zip(T._RNN_KEYS, T._GRU_NAMES)})
        self.dh = torch.randn(P, 2 * Hd, generator=_gen("engine-gru-upstream", self.id))
        self._ref = None

    def loader_kwargs(self, d):
        """kwargs of GruLayer.fwd / bwd for the device tensors d"""
        kw = {}
        if "scale" in d:
            kw.update(in_scale=d["scale"], in_shift=d["shift"])
        if "strip" in d:
            kw.update(in_b=d["strip"], cin_a=self.cin_a)
        if "x2" in d:
            kw.update(in2=d["x2"])
        return kw

    def loader_out(self, dtype):
        """what the loader hands to the projection: [N][H][W][Cin]"""
        N, H, W, ca = self.N, self.H, self.W, self.cin_a
        d = {k: v.to(dtype) for k, v in self.ins.items()}
        a = d["x"].view(N, H, W, ca)
        if "scale" in d:
            a = a * d["scale"][:ca] + d["shift"][:ca]
        if "x2" in d:
            a = a + d["x2"].view(N, H, W, ca)
        if "strip" in d:
            a = torch.cat([a, d["strip"].view(N, 1, W, STRIP).expand(N, H, W, STRIP)], -1)
        return a

    def reference(self):
        """{h, dx, every parameter gradient} in float64: computed once and never modified"""
        if self._ref is not None:
            return self._ref
        dtype = F64
        N, H, W, U, Hd = self.N, self.H, self.W, self.U, self.Hd
        a = self.loader_out(dtype).clone().requires_grad_(True)
        p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in self.params.items()}
        y = F.conv2d(a.permute(0, 3, 1, 2), p["conv1.weight"], p["conv1.bias"]).permute(0, 2, 3, 1)          # [N][H][W][U]
        d = {n: p["gru." + k] for k, n in zip(T._RNN_KEYS, T._GRU_NAMES)}
        if self.axis == 0:
            h = T._rnn_ref(torch.nn.GRU, y.reshape(N * H, W, U), d, Hd).reshape(N, H, W, 2 * Hd)
        else:
            h = T._rnn_ref(torch.nn.GRU, y.permute(0, 2, 1, 3).reshape(N * W, H, U), d, Hd).reshape(N, W, H, 2 * Hd).permute(0, 2, 1, 3)
        h = h.reshape(self.P, 2 * Hd)
        h.backward(self.dh.to(dtype))
        out = {"h": h.detach(), "dx": a.grad.reshape(self.P, self.Cin)}
        out.update({k: p[k].grad for k in GRU_KEYS})
        self._ref = out
        return out

    # -- what the engine is expected to launch (GruLayer's docstrings) --
    def fused_forward(self, policy):
        T_, nseq = (self.W, self.N * self.H) if self.axis == 0 else (self.H, self.N * self.W)
        return bool(TERMS[policy]) and self.Hd == 32 and self.Cin in (64, 96) and (T_ == 64 or (T_ == 16 and nseq % 4 == 0))

    def fused_wgrad(self, policy):
        return bool(TERMS[policy]) and self.Hd == 32

    def expected_launches(self, policy, passes=1):
        u = "" if self.Hd == 32 else "_u"
        fwd = ["tpgsr_bigru_proj_fwd"] if self.fused_forward(policy) else ["tpgsr_conv_fwd", "tpgsr_bigru_fwd" + u]
        if self.fused_wgrad(policy):
            bwd = ["tpgsr_bigru_bwd2", "tpgsr_gru_wgrad"] + ["tpgsr_wgrad_reduce"] * 3 + ["tpgsr_conv_fwd"]
        else:
            bwd = ["tpgsr_bigru_bwd" + u] + ["tpgsr_conv_wgrad", "tpgsr_wgrad_reduce"] * 3 + ["tpgsr_conv_fwd"]
        return _pack_names(policy) + fwd + (bwd + ["tpgsr_compose_bwd_program"]) * passes


def gru_cases():
    return [GruCase(*L, *m) for L in GRU_LAYERS for m in GRU_MAPS]


def gru_holder(case):
    """a module with the reference's GruBlock under the prefix `g`, holding the case's parameters"""
    from tpgsr_amd.model import tsrn

    class Holder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.g = tsrn.GruBlock(case.Cin, case.U)
    m = Holder()
    with torch.no_grad():
        have = dict(m.named_parameters())
        assert set(have) == {"g." + k for k in case.params}, sorted(have)
        for k, v in case.params.items():
            assert have["g." + k].shape == v.shape, (k, tuple(have["g." + k].shape), tuple(v.shape))
            have["g." + k].copy_(v)
    return m


def run_gru(case, device, split_dh=False, passes=1):
    """the engine's GruLayer on the case: ({h, dx, parameter gradients} on the CPU, the launches, the engine, the device tensors).
    split_dh: the upstream gradient arrives as two tensors (dh, dh2); passes: `bwd` + `flush_compose_bwd` that many times on one arena"""
    engine = _engine_base()
    eng = OneLayerEngine(gru_holder(case), lambda e: engine.GruLayer(e, "g", case.axis))
    P, Hd, Cin = case.P, case.Hd, case.Cin
    d = {k: v.to(device).contiguous() for k, v in case.ins.items()}
    kw = case.loader_kwargs(d)
    nan = lambda *s: torch.full(s, float("nan"), device=device)
    buf = dict(gi=nan(P, 6 * Hd), h=nan(P, 2 * Hd), gates=nan(P, 8 * Hd), dgi=nan(P, 6 * Hd), dgh=nan(P, 6 * Hd), dx=nan(P, Cin))
    if split_dh:
        part = torch.randn(P, 2 * Hd, generator=_gen("engine-gru-split", case.id))
        dh, dh2 = (case.dh - part).to(device), part.to(device)
    else:
        dh, dh2 = case.dh.to(device), None

    def fn(eng, L):
        L.fwd(case.N, case.H, case.W, d["x"], buf["gi"], buf["h"], buf["gates"], **kw)
        for i in range(passes):
            if i:
                eng.flush_compose_bwd()
            L.bwd(case.N, case.H, case.W, d["x"], buf["gates"], buf["h"], dh, dh2, buf["dgi"], buf["dgh"], buf["dx"], **kw)

    with launch_log() as names:
        eng.run(fn, device)
    got = {"h": buf["h"].cpu(), "dx": buf["dx"].cpu()}
    for k, v in case.params.items():
        got[k] = eng.G["g." + k].cpu().view(v.shape)
    d.update(buf)
    return got, names, eng, d


# ---- TConvStrip / FoldedDgrad ------------------------------------------------------------------------------------------------
class _ParamHolder(torch.nn.Module):
    """the parameter `w`, then `guard`: the next tensor of the arena, four of w's leading slices wide (more than the channels a layer pads
    w's operands with), whose gradient nothing may touch"""

    def __init__(self, w):
        super().__init__()
        self.w = torch.nn.Parameter(w.clone())
        self.guard = torch.nn.Parameter(torch.zeros(4 * (w.numel() // w.shape[0])))


def _guard_untouched(eng, w):
    """the arena holds exactly w's gradient, then the guard's, and the guard's is still zero: nothing was written past the end of w's"""
    o = eng.arena.offsets
    assert eng.G["w"].numel() == w.numel() and o["guard"] == o["w"] + (w.numel() + 3) // 4 * 4
    assert not bool(eng.G["guard"].cpu().any()), "a gradient was written past the end of the parameter's"


class StripCase:
    """ConvTranspose2d(Cin, Cout, 3, stride (2, sw), padding (1, pw), bias=False) on the strip [N][1][Win][Cin]"""

    def __init__(self, Cin, Cout, sw, pw, N, Win):
        self.Cin, self.Cout, self.sw, self.pw, self.N, self.Win = Cin, Cout, sw, pw, N, Win
        self.id = f"tconv-{Cin}to{Cout}-s{sw}p{pw}-{N}x{Win}"
        self.OW = (Win - 1) * sw - 2 * pw + 3
        g = _gen("engine-strip", self.id)
        self.w = torch.randn(Cin, Cout, 3, 3, generator=g) / (3 * Cin) ** 0.5
        self.x = torch.randn(N * Win, Cin, generator=g)
        self.dy = torch.randn(N * self.OW, Cout, generator=g)
        self._ref = None

    def reference(self):
        if self._ref is not None:
            return self._ref
        dtype = F64
        N, Win = self.N, self.Win
        x = self.x.to(dtype).view(N, 1, Win, self.Cin).permute(0, 3, 1, 2).clone().requires_grad_(True)
        w = self.w.to(dtype).clone().requires_grad_(True)
        y = F.conv_transpose2d(x, w, stride=(2, self.sw), padding=(1, self.pw))
        assert tuple(y.shape) == (N, self.Cout, 1, self.OW), tuple(y.shape)
        y.backward(self.dy.to(dtype).view(N, 1, self.OW, self.Cout).permute(0, 3, 1, 2))
        out = {"y": y.detach().permute(0, 2, 3, 1).reshape(N * self.OW, self.Cout), "dx": x.grad.permute(0, 2, 3, 1).reshape(N * Win, self.Cin),
               "dw": w.grad}
        self._ref = out
        return out

    def expected_launches(self, policy):
        pad = ["tpgsr_pad_channels"] if self.Cin % 4 else []
        red = "tpgsr_wgrad_reduce_program" if self.Cin % 4 else "tpgsr_wgrad_reduce"
        return _pack_names(policy) + pad + ["tpgsr_conv_fwd", "tpgsr_conv_wgrad", red, "tpgsr_conv_fwd"]


STRIP_CASES = [(37, 64, 2, 1, 2, 26), (64, 32, 1, 0, 2, 7)]


def strip_cases():
    return [StripCase(*c) for c in STRIP_CASES]


def run_strip(case, device):
    from tpgsr_amd import kernels as K
    engine = _engine_base()
    eng = OneLayerEngine(_ParamHolder(case.w), lambda e: engine.TConvStrip(e, "w", case.sw, case.pw))
    N, Win = case.N, case.Win
    x, dy = case.x.to(device), case.dy.to(device)
    y, dx = torch.full((N * case.OW, case.Cout), float("nan"), device=device), torch.full((N * Win, case.Cin), float("nan"), device=device)

    def fn(eng, L):
        xin = x
        if L.Cp != L.Cin:          # the caller hands in the strip padded to Cp channels (engine._record_infogen_fwd)
            xin = torch.full((N * Win, L.Cp), float("nan"), device=device)
            K.pad_channels(x, N * Win, L.Cin, L.Cp, xin)
        assert L.out_w(Win) == case.OW
        L.fwd(N, Win, xin, y)
        L.wgrad(N, Win, xin, dy)
        L.dgrad(N, Win, dy, dx)

    with launch_log() as names:
        eng.run(fn, device)
    _guard_untouched(eng, case.w)
    return {"y": y.cpu(), "dx": dx.cpu(), "dw": eng.G["w"].cpu().view(case.w.shape)}, names


class FoldCase:
    """the data gradient of Conv2d(Ci, Cout, KS, padding=KS // 2) on an [N][H][W] map"""

    def __init__(self, Cout, Ci, KS, N, H, W):
        self.Cout, self.Ci, self.KS, self.N, self.H, self.W = Cout, Ci, KS, N, H, W
        self.id = f"fold-{Cout}x{Ci}x{KS}-{N}x{H}x{W}"
        g = _gen("engine-fold", self.id)
        self.w = torch.randn(Cout, Ci, KS, KS, generator=g) / (KS * KS * Ci) ** 0.5
        self.dy = torch.randn(N * H * W, Cout, generator=g)
        self._ref = None

    def reference(self):
        if self._ref is not None:
            return self._ref
        dtype = F64
        N, H, W = self.N, self.H, self.W
        x = torch.zeros(N, self.Ci, H, W, dtype=dtype, requires_grad=True)
        y = F.conv2d(x, self.w.to(dtype), padding=self.KS // 2)
        y.backward(self.dy.to(dtype).view(N, H, W, self.Cout).permute(0, 3, 1, 2))
        out = {"dx": x.grad.permute(0, 2, 3, 1).reshape(N * H * W, self.Ci)}
        self._ref = out
        return out

    def expected_launches(self, policy):
        return _pack_names(policy) + ["tpgsr_conv_fwd", "tpgsr_shiftsum_nhwc"]


FOLD_CASES = [(64, Ci, 9, *m) for Ci in (4, 3) for m in ((1, 16, 64), (2, 5, 7))]


def fold_cases():
    return [FoldCase(*c) for c in FOLD_CASES]


def run_fold(case, device):
    engine = _engine_base()
    eng = OneLayerEngine(_ParamHolder(case.w), lambda e: engine.FoldedDgrad(e, "w"))
    P = case.N * case.H * case.W
    dy = case.dy.to(device)
    scratch, dx = torch.full((P, case.KS * case.Ci), float("nan"), device=device), torch.full((P, case.Ci), float("nan"), device=device)
    with launch_log() as names:
        eng.run(lambda eng, L: L.run(case.N, case.H, case.W, dy, scratch, dx), device)
    _guard_untouched(eng, case.w)
    return {"dx": dx.cpu()}, names


# ---- the chain rule and the composed operand, called directly -------------------------------------------------------------
COMPOSE_SHAPES = [(64, 64, 96), (96, 64, 96), (160, 128, 192), (4, 4, 3)]       # (Cin, U, G)
COMPOSE_OUT = ("dW1", "db1", "dwih0", "dwih1", "dbih0", "dbih1")


def compose_case(Cin, U, G):
    """inputs, seeded non-zero pre-fill of every output, and the float64 / float32 references (pre-fill included)"""
    g = _gen("compose", Cin, U, G)
    r = lambda *s: torch.randn(*s, generator=g)
    t = dict(dWc=r(2 * G, Cin), dbc=r(2 * G), W1=r(U, Cin) / Cin ** 0.5, b1=r(U) * 0.5, wih0=r(G, U) / U ** 0.5, wih1=r(G, U) / U ** 0.5)
    fill = dict(dW1=r(U, Cin), db1=r(U), dwih0=r(G, U), dwih1=r(G, U), dbih0=r(G), dbih1=r(G))

    def ref(dtype):
        p = {k: t[k].to(dtype).clone().requires_grad_(True) for k in ("W1", "b1", "wih0", "wih1")}
        bih = torch.zeros(2 * G, dtype=dtype, requires_grad=True)
        wih = torch.cat([p["wih0"], p["wih1"]])
        Wc, bc = wih @ p["W1"], wih @ p["b1"] + bih
        torch.autograd.backward([Wc, bc], [t["dWc"].to(dtype), t["dbc"].to(dtype)])
        f = {k: v.to(dtype) for k, v in fill.items()}
        return {"dW1": f["dW1"] + p["W1"].grad, "db1": f["db1"] + p["b1"].grad, "dwih0": f["dwih0"] + p["wih0"].grad,
                "dwih1": f["dwih1"] + p["wih1"].grad, "dbih0": f["dbih0"] + bih.grad[:G], "dbih1": f["dbih1"] + bih.grad[G:]}
    return t, fill, ref(F64), ref(torch.float32)


def composed_case(Cin, U, G):
    """kinds 5 / 6: both directions' W_ih [G][U], b_ih [G], conv1 W1 [U][Cin], b1 [U]; float64 / float32 Wc [2G][Cin] and bc [2G]"""
    g = _gen("composed", Cin, U, G)
    r = lambda *s: torch.randn(*s, generator=g)
    t = dict(wih0=r(G, U) / U ** 0.5, wih1=r(G, U) / U ** 0.5, bih0=r(G), bih1=r(G), W1=r(U, Cin) / Cin ** 0.5, b1=r(U))

    def ref(dtype):
        d = {k: v.to(dtype) for k, v in t.items()}
        wih = torch.cat([d["wih0"], d["wih1"]])
        return {"Wc": wih @ d["W1"], "bc": wih @ d["b1"] + torch.cat([d["bih0"], d["bih1"]])}
    return t, ref(F64), ref(torch.float32)


def arith_bound(ref32, ref64):
    """the suite's `arith` rule: 4 x the error of float32 PyTorch on the CPU + 4 * 2^-24"""
    return 4 * err(ref32, ref64) + FLOOR
