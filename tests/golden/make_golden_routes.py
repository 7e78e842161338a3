"""Generator of tests/golden/conv_routes.json: which kernel tpgsr_conv_fwd / tpgsr_conv_wgrad choose (tpgsr_conv_route /
tpgsr_conv_wgrad_route) and what the planners answer, over

  * a deterministic sweep of argument blocks built directly as ConvArgs / WgradArgs with dummy aligned pointers (geometry, loader
    bits, terms, strides, split counts, and every switch a test can reach at both settings), and
  * every argument block the dry-run plans of the engines record: the TSRN_TL + CRNN cascade step at the bench's C3 shape (batch 48)
    and one `_TL` backbone, each under f32 / x3 / x2 / bf16.

The committed file was first written by the commit BEFORE the route function existed, from a probe that called that commit's own launcher
predicates in the launchers' order: tests/test_conv_route_cpu.py holds every later commit to it, field for field.  Host only, no GPU.

    python tests/golden/make_golden_routes.py            # rewrite the golden file
    python tests/golden/make_golden_routes.py --emit sweep,recorded     # (the test's subprocess) print sections' results as JSON
"""
import ctypes as C
import itertools
import json
import os
import subprocess
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
GOLDEN = os.path.join(HERE, "conv_routes.json")
sys.path.insert(0, ROOT)

PTR = 0x10000000          # dummy operand addresses: 16-byte aligned, never dereferenced
PTR_FIELDS = {"in_", "in2", "in_scale", "in_shift", "wt", "bias", "out", "bn_partial", "in_b", "wt_bf", "bnb_y", "bnb_mean", "bnb_rstd", "bnb_scale",
              "bnb_shift", "in2_scale", "sk_part", "dy", "part", "dbpart", "dy_bf"}
FWD_FIELDS = ("kernel", "ld", "lcap", "nbw", "lds_bytes", "splits", "sk_plan")
WG_FIELDS = ("kernel", "ld", "lcap", "ne", "lds_bytes", "Z", "MB", "vecY")
# switches a test can reach and the route reads: (setter, default, other setting)
KNOBS = {"halo3": ("tpgsr_halo3_set_enabled", 1, 0), "panel": ("tpgsr_panel_set_enabled", 1, 0), "panel_min_m": ("tpgsr_panel_set_min_m", 32768, 64),
         "panel_k192": ("tpgsr_panel_set_k192", 0, 1), "wgrad3": ("tpgsr_wgrad3_set_enabled", 1, 0), "splitk": ("tpgsr_splitk_set_enabled", 1, 0),
         "min_taps": ("tpgsr_halo_set_min_taps", 2, 1)}


def _lib():
    from tpgsr_amd import _lib as L
    return L, L.load()


def conv_args(N, H, W, Cin, Cout, KH=1, KW=1, pad_h=0, pad_w=0, *, terms=0, ld=0, OH=None, OW=None, cin_order=None, **kw):
    """one ConvArgs; `ld`: loader bits to set up operands for (1 affine, 2 activation, 4 residual, 8 pixel-shuffle gather, 16 strip,
    32 scaled residual); cin_order: wt_bf_cin (default: Cin when Cin % 32 == 0 and the convolution has more than one tap, as the engines do)"""
    L, _ = _lib()
    a = L.ConvArgs()
    a.in_, a.wt, a.out = PTR, PTR + 0x1000, PTR + 0x2000
    a.N, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW, a.pad_h, a.pad_w = N, H, W, Cin, Cout, KH, KW, pad_h, pad_w
    a.OH = H + 2 * pad_h - KH + 1 if OH is None else OH
    a.OW = W + 2 * pad_w - KW + 1 if OW is None else OW
    a.in_ld, a.in2_ld, a.out_ld = Cin, Cin, Cout
    a.in_dil_w = a.stride_w = 1
    if ld & 1:
        a.in_scale, a.in_shift = PTR + 0x3000, PTR + 0x3100
    if ld & 2:
        a.in_act = 2
    if ld & 4:
        a.in2 = PTR + 0x4000
    if ld & 8:
        a.in_ps = 1
    if ld & 16:
        a.in_b, a.cin_a, a.in_b_ld = PTR + 0x5000, Cin // 2, Cin - Cin // 2
        a.in_ld = Cin // 2
    if ld & 32:
        a.in2_scale = PTR + 0x3200
    a.terms = terms
    if terms and Cin % 4 == 0:
        a.kp = (KH * KW * Cin + 31) // 32 * 32
        a.wt_bf = PTR + 0x6000
        a.wt_bf_cin = (Cin if (Cin % 32 == 0 and KH * KW > 1) else 0) if cin_order is None else cin_order
    for k, v in kw.items():
        assert hasattr(a, k), k
        setattr(a, k, v)
    return a


def wgrad_args(a, *, dy_ld=None, dy_coff=0, dy_ps=0, zsplits=0, dy_bf=0, dy=PTR + 0x7000):
    L, _ = _lib()
    w = L.WgradArgs()
    w.c = a
    w.dy, w.part = dy, PTR + 0x8000
    w.dy_ld = a.Cout if dy_ld is None else dy_ld
    w.dy_coff, w.dy_ps, w.zsplits, w.dy_bf = dy_coff, dy_ps, zsplits, dy_bf
    return w


TAPS = ((1, 1, 0, 0), (2, 2, 0, 0), (3, 3, 1, 1), (9, 9, 4, 4), (1, 3, 0, 1))
OWS = (6, 7, 8, 16, 26, 50, 64, 65, 128)
CHANNELS = (4, 32, 37, 64, 96, 128, 192, 256, 512)
CH_PAIRS = ((4, 64), (32, 64), (37, 64), (64, 64), (64, 37), (64, 96), (96, 192), (64, 256), (128, 64), (192, 64), (192, 32), (256, 512), (512, 128))
FWD_LDS = (0, 1, 2, 3, 4, 5, 7, 8, 17, 37, 6, 9, 16, 21, 33, 36)      # what the launchers accept, then a few they reject
WG_LDS = (0, 1, 2, 3, 4, 5, 7, 17, 6, 8, 16)


def _batches(OH, OW, Cout):
    """batch sizes that put M = N OH OW on either side of the panel's minimum M (32768), of 192 whole-CU super-tiles and of 256 split-K tiles"""
    px, nbn = OH * OW, (Cout + 63) // 64
    out = {48}
    for m in (32768, 192 * 192 // nbn, 256 * 64 // nbn):
        n = max(1, m // px)
        out.update((n, n + 1))
    return sorted(out)


def sweep():
    """[(op, args, knobs)]: deterministic, in a fixed order.  Not a cross product: every value of the issue's lists appears, each list is
    crossed with the lists it interacts with, and the rest cycles."""
    cases = []
    add = lambda op, a, **knobs: cases.append((op, a, knobs))
    bf = PTR + 0x9000
    # geometry: every tap shape x map width x terms, channel pairs cycling
    for i, ((KH, KW, ph, pw), OW, terms) in enumerate(itertools.product(TAPS, OWS, (0, 1, 2, 3))):
        for Ci, Co in (CH_PAIRS[i % 13], CH_PAIRS[(5 * i + 3) % 13]):
            add("fwd", conv_args(48, 16 if KH <= 3 else 12, OW, Ci, Co, KH, KW, ph, pw, terms=terms))
    # M on either side of the panel's minimum, of 192 whole-CU super-tiles and of 256 split-K tiles
    for (KH, KW, ph, pw), (Ci, Co), terms in itertools.product(TAPS, ((64, 64), (64, 96), (256, 512)), (1, 2, 3)):
        for OW in (64, 26) if KH == 3 else (64,):
            for N in _batches(16 if KH <= 3 else 12, OW, Co):
                add("fwd", conv_args(N, 16 if KH <= 3 else 12, OW, Ci, Co, KH, KW, ph, pw, terms=terms))
    # all channel counts on both sides
    for Ci, Co in itertools.product(CHANNELS, CHANNELS):
        add("fwd", conv_args(48, 16, 64, Ci, Co, terms=2))
        add("fwd", conv_args(48, 16, 64, Ci, Co, 3, 3, 1, 1, terms=2))
        add("wgrad", wgrad_args(conv_args(48, 16, 64, Ci, Co, 3, 3, 1, 1, terms=2)))
        if Ci == Co:
            for t in (TAPS[0], TAPS[2]):
                add("fwd", conv_args(48, 16, 64, Ci, Co, *t))
                add("wgrad", wgrad_args(conv_args(48, 16, 64, Ci, Co, *t)))
    # loader bits x terms x a shape for every kernel family (trunk 3x3, small-map 3x3, projection 1x1, strip 1x3, short 3x3, long-K 1x1)
    shapes = ((48, 16, 64, 64, 64, 3, 3, 1, 1), (48, 4, 26, 256, 512, 3, 3, 1, 1), (48, 16, 64, 64, 192, 1, 1, 0, 0), (48, 1, 26, 128, 64, 1, 3, 0, 1),
              (2, 8, 16, 32, 64, 3, 3, 1, 1), (48, 1, 26, 2048, 512, 1, 1, 0, 0))
    for shp, ld, terms in itertools.product(shapes, FWD_LDS, (0, 1, 2, 3)):
        add("fwd", conv_args(*shp, terms=terms, ld=ld))
        if ld in (4, 5, 7) and terms == 2:
            add("fwd", conv_args(*shp, terms=terms, ld=ld, out_ps=1))
        if shp in shapes[:2] and terms == 2:
            add("fwd", conv_args(*shp, terms=terms, ld=ld), halo3=0)
    for shp, ld, terms in itertools.product(shapes[:4], WG_LDS, (0, 1, 2, 3)):
        a = conv_args(*shp, terms=terms, ld=ld)
        for z, b in ((16, bf),) if terms in (1, 3) else ((0, 0), (16, 0), (16, bf), (0, bf)):
            add("wgrad", wgrad_args(a, zsplits=z, dy_bf=b))
    # the other argument fields, one at a time over a shape each kernel would otherwise take
    for shp, terms in itertools.product(shapes, (0, 2, 3)):
        if terms == 3 and shp not in shapes[:2]:
            continue
        Ci, Co = shp[3], shp[4]
        for kw in (dict(out_ps=1), dict(ld=16), dict(in_dil_w=2), dict(stride_w=2), dict(cin_order=0), dict(cin_order=Ci), dict(wt_coff=32, wt_ld=Co + 32),
                   dict(wt_coff=4, wt_ld=Co + 32), dict(wt_ld=Co + 1), dict(wt=PTR + 0x1004), dict(in_coff=4, in_ld=Ci + 4), dict(bn_row_tiles=3),
                   dict(sk_splits=4, sk_part=PTR + 0xa000), dict(sk_splits=4, sk_part=PTR + 0xa000, ld=37), dict(sk_splits=1), dict(out_act=1),
                   dict(OH=max(1, shp[1] - 1)), dict(kp=192) if shp[5] * shp[6] == 1 else dict(kp=0)):
            add("fwd", conv_args(*shp, terms=terms, **kw))
        if terms == 3:
            continue
        a = conv_args(*shp, terms=terms)
        for kw in (dict(dy_ps=1), dict(dy_ld=Co + 4), dict(dy_ld=Co + 4, dy_coff=4), dict(dy_ld=Co + 1), dict(dy=PTR + 0x7004), dict(zsplits=3),
                   dict(zsplits=8, dy_bf=bf, dy_ps=1), dict(dy_ld=(Co + 3) // 4 * 4 + 4, dy_coff=2)):
            add("wgrad", wgrad_args(a, **kw))
        for kw in (dict(in_dil_w=2), dict(stride_w=2), dict(ld=8), dict(ld=16)):
            add("wgrad", wgrad_args(conv_args(*shp, terms=terms, **kw), zsplits=8, dy_bf=bf))
    # every output width under the weight-gradient halo kernel (7- and 9-entry variants) and the 37-class head
    for OW, Ci, Co, terms in itertools.product(OWS, (64, 256), (128, 37), (2, 3)):
        a = conv_args(48, 8, OW, Ci, Co, 3, 3, 1, 1, terms=terms)
        add("wgrad", wgrad_args(a, zsplits=12, dy_bf=bf, dy_ld=(Co + 3) // 4 * 4))
    # every switch a test can reach, at its other setting, over shapes on both sides of what it moves
    knob_shapes = shapes + ((48, 16, 64, 64, 96, 1, 1, 0, 0), (2, 16, 64, 64, 64, 1, 1, 0, 0), (48, 16, 64, 192, 64, 1, 1, 0, 0), (8, 2, 39, 64, 128, 2, 2, 0, 0),
                            (1, 6, 16, 256, 256, 3, 3, 1, 1))
    for name, shp in itertools.product(KNOBS, knob_shapes):
        other = {name: KNOBS[name][2]}
        add("fwd", conv_args(*shp, terms=2), **other)
        add("fwd", conv_args(*shp, terms=1), **other)
        add("fwd", conv_args(*shp, terms=2, cin_order=0), **other)
        add("wgrad", wgrad_args(conv_args(*shp, terms=2), zsplits=8, dy_bf=bf), **other)
    for shp, terms in itertools.product(knob_shapes, (2, 3)):          # two switches that meet: 1x1 convolutions the halo AND the panel kernel take
        add("fwd", conv_args(*shp, terms=terms, cin_order=0), min_taps=1, panel_min_m=64)
    return cases


def minwork_sweep():
    """the weight-gradient halo kernel's Cin x Cout threshold (TPGSR_XBF_WGRAD_HALO_MINWORK, read when the library loads): run with it at 0"""
    cases = []
    for (Ci, Co), OW in itertools.product(CH_PAIRS, (8, 64)):
        a = conv_args(48, 16, OW, Ci, Co, 3, 3, 1, 1, terms=2)
        cases.append(("wgrad", wgrad_args(a, zsplits=8, dy_bf=PTR + 0x9000, dy_ld=(Co + 3) // 4 * 4), {}))
        cases.append(("halo_plan", a, {}))
    return cases


def fields_of(st):
    """the non-zero fields of a ctypes argument block (nested for WgradArgs.c), pointers as integers"""
    out = {}
    for name, *_ in st._fields_:
        v = getattr(st, name)
        if isinstance(v, C.Structure):
            out[name] = fields_of(v)
        elif v:
            out[name] = v
    return out


def evaluate(op, args, knobs):
    """(argument block bytes, [route fields..., planner answers...]) of one case"""
    L, lib = _lib()
    for k, v in knobs.items():
        getattr(lib, KNOBS[k][0])(v)
    try:
        rec = []
        if op == "fwd":
            r = L.ConvRoute()
            assert lib.tpgsr_conv_route(C.byref(args), C.byref(r)) == r.kernel
            nb = C.c_longlong(0)
            rec += [getattr(r, f) for f in FWD_FIELDS]
            S = lib.tpgsr_conv_splitk_plan(C.byref(args), C.byref(nb))
            rec += [S, nb.value, lib.tpgsr_conv_bn_row_tiles(C.byref(args)), lib.tpgsr_conv_in2_scale_ok(C.byref(args)),
                    lib.tpgsr_halo_capacity(C.byref(args))]
            taken = L.ConvRoute()          # the planner's proposal, taken: what the launcher then runs
            if S > 1:
                b = L.ConvArgs.from_buffer_copy(args)
                b.sk_splits, b.sk_part = S, PTR + 0xa000
                lib.tpgsr_conv_route(C.byref(b), C.byref(taken))
            rec += [taken.kernel, taken.splits]
        elif op == "wgrad":
            r = L.WgradRoute()
            assert lib.tpgsr_conv_wgrad_route(C.byref(args), C.byref(r)) == r.kernel
            rec += [getattr(r, f) for f in WG_FIELDS]
            z, nb = C.c_int(0), C.c_longlong(0)
            rec += [lib.tpgsr_wgrad_halo_plan(C.byref(args.c), C.byref(z), C.byref(nb)), z.value, nb.value,
                    lib.tpgsr_wgrad_splits(args.c.N * args.c.OH * args.c.OW, args.c.KH * args.c.KW * args.c.Cin, args.c.Cout)]
        else:
            z, nb = C.c_int(0), C.c_longlong(0)
            rec += [lib.tpgsr_wgrad_halo_plan(C.byref(args), C.byref(z), C.byref(nb)), z.value, nb.value]
        return bytes(args), rec
    finally:
        for k in knobs:
            getattr(lib, KNOBS[k][0])(KNOBS[k][1])


RECORD = r'''
import ctypes as C, json, sys, torch
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(here)r)
from tpgsr_amd import kernels as K
assert K.DRYRUN
import make_golden_routes as G
from tpgsr_amd.interfaces.super_resolution import TPGSRTrainStep
from tpgsr_amd.model import srresnet, tsrn
from tpgsr_amd.model.crnn import crnn

def norm(d):          # addresses differ from run to run: keep what a route can depend on, their alignment
    return {k: norm(v) if isinstance(v, dict) else ((G.PTR | (v & 15)) if k in G.PTR_FIELDS else v) for k, v in d.items()}
seen, out = set(), []
torch.manual_seed(0)
N = 48
for prec in ("f32", "x3", "x2", "bf16"):
    for make, crit in ((lambda: tsrn.TSRN_TL(STN=True, mask=True), None),
                       (lambda: srresnet.SRResNet_TL(scale_factor=2, width=128, height=32, STN=False, mask=True), "mse")):
        net = make().train()
        stu, teacher = crnn.CRNN(32, 1, 37, 256).train(), crnn.CRNN(32, 1, 37, 256).eval()
        kw = dict(image_crit=crit) if crit else {}
        ts = TPGSRTrainStep([net], [stu], teacher, stu_iter=1, precision=prec, **kw)
        ts.step(torch.rand(N, 4, 16, 64), torch.rand(N, 4, 32, 128))
        for m in (net, stu, teacher):
            for pl in m._engine()._plans.values():
                for plan in [v for k, v in pl.items() if hasattr(v, "ops")]:
                    blocks = []
                    for i, (name, fn, args, sid) in enumerate(plan.ops):
                        if name in ("tpgsr_conv_fwd", "tpgsr_conv_wgrad"):
                            blocks.append(("fwd" if name == "tpgsr_conv_fwd" else "wgrad", args[0]._obj))
                        elif name == "tpgsr_conv_wgrad_batch":
                            blocks += [("wgrad", w) for w in getattr(plan, 'meta', {}).get(i, [])]
                    for op, st in blocks:
                        d = norm(G.fields_of(st))
                        key = op + json.dumps(d, sort_keys=True)
                        if key not in seen:
                            seen.add(key)
                            out.append([op, d])
print("RESULT " + json.dumps(out))
'''


def recorded():
    """[[op, fields]] of every distinct tpgsr_conv_fwd / tpgsr_conv_wgrad argument block the engines' dry-run plans hold"""
    env = dict({k: v for k, v in os.environ.items() if not k.startswith("TPGSR_")}, TPGSR_PLAN_DRYRUN="1")
    r = subprocess.run([sys.executable, "-c", RECORD % dict(root=ROOT, here=HERE)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


def pack_blocks(blocks):
    """[[op, fields]] -> {op: {"fields": [dotted names], "rows": [[values]]}, "order": "fw..."}; a pointer is 0 (null) or 1 + its low four bits"""
    flat = lambda d, pre="": {pre + k: x for k, v in d.items() for k, x in (flat(v, k + ".").items() if isinstance(v, dict) else ((k, v),))}
    out = {"order": "".join(op[0] for op, _ in blocks)}
    for op in ("fwd", "wgrad"):
        ds = [flat(d) for o, d in blocks if o == op]
        names = sorted({k for d in ds for k in d})
        enc = lambda k, v: (1 + (v & 15) if v else 0) if k.split(".")[-1] in PTR_FIELDS else v
        rows = [[enc(k, d.get(k, 0)) for k in names] for d in ds]
        const = {k: rows[0][i] for i, k in enumerate(names) if all(r[i] == rows[0][i] for r in rows)}      # fields no block varies: once
        keep = [i for i, k in enumerate(names) if k not in const]
        out[op] = {"const": const, "fields": [names[i] for i in keep], "rows": [[r[i] for i in keep] for r in rows]}
    return out


def recorded_cases(packed):
    L, _ = _lib()
    its = {op: iter(packed[op]["rows"]) for op in ("fwd", "wgrad")}
    cases = []
    for o in packed["order"]:
        op = "fwd" if o == "f" else "wgrad"
        st = (L.ConvArgs if op == "fwd" else L.WgradArgs)()
        for k, v in list(packed[op]["const"].items()) + list(zip(packed[op]["fields"], next(its[op]))):
            tgt, leaf = (st.c, k[2:]) if k.startswith("c.") else (st, k)
            setattr(tgt, leaf, (PTR | (v - 1) if v else 0) if leaf in PTR_FIELDS else v)
        cases.append((op, st, {}))
    return cases


def cases_of(section, blocks=None):
    if section == "recorded":
        if blocks is None:
            blocks = load_golden()["recorded_blocks"]
        return recorded_cases(blocks)
    return {"sweep": sweep, "minwork0": minwork_sweep}[section]()


def emit(section, blocks=None):
    cases = cases_of(section, blocks)
    res = [evaluate(*c) for c in cases]
    # (args_crc: the argument blocks these rows belong to, so that a changed sweep is told apart from a changed route)
    return {"args_crc": zlib.crc32(b"".join(b for b, _ in res)), "rows": [r for _, r in res]}


def dedup(rows):
    """rows repeat: the file keeps each distinct row once ("uniq") and the rows as indices into that list ("idx")"""
    uniq = sorted({tuple(r) for r in rows})
    at = {r: i for i, r in enumerate(uniq)}
    return {"uniq": [list(r) for r in uniq], "idx": [at[tuple(r)] for r in rows]}


def expand(d):
    return [d["uniq"][i] for i in d["idx"]]


def load_golden():
    with open(GOLDEN) as f:
        gold = json.load(f)
    for sec in ("sweep", "recorded", "minwork0"):
        if sec in gold:
            gold[sec]["rows"] = expand(gold[sec]["rows"])
    return gold


def run_emit(sections, **env):
    """{section: emit(section)} from a fresh process whose environment holds none of the library's switches but `env`: ConvKnobs is
    initialised when the library loads, and a test module of the suite sets one of them for its whole process"""
    clean = {k: v for k, v in os.environ.items() if not k.startswith("TPGSR_")}
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--emit", ",".join(sections)], capture_output=True, text=True, env=dict(clean, **env))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


def main():
    if "--emit" in sys.argv:
        print("RESULT " + json.dumps({s: emit(s) for s in sys.argv[sys.argv.index("--emit") + 1].split(",")}))
        return
    blocks = pack_blocks(recorded())
    gold = {"fwd_fields": list(FWD_FIELDS) + ["splitk_plan", "sk_bytes", "bn_row_tiles", "in2_scale_ok", "halo_capacity", "sk_taken_kernel", "sk_taken_splits"],
            "wgrad_fields": list(WG_FIELDS) + ["halo_plan", "halo_zsplits", "dy_bf_bytes", "wgrad_splits"], "recorded_blocks": blocks}
    with open(GOLDEN, "w") as f:      # (the fresh process reads the recorded blocks from the file)
        json.dump(gold, f)
    gold.update(run_emit(["sweep", "recorded"]))
    gold.update(run_emit(["minwork0"], TPGSR_XBF_WGRAD_HALO_MINWORK="0"))
    n_sweep = len(gold["sweep"]["rows"])
    for sec in ("sweep", "recorded", "minwork0"):
        gold[sec]["rows"] = dedup(gold[sec]["rows"])
    with open(GOLDEN, "w") as f:
        json.dump(gold, f, separators=(",", ":"))
        f.write("\n")
    print(f"{GOLDEN}: {n_sweep} sweep cases, {len(blocks['order'])} recorded blocks, {os.path.getsize(GOLDEN)} bytes")


if __name__ == "__main__":
    main()
