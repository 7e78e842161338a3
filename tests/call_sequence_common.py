"""What tests/test_call_sequences_gpu.py and tests/test_call_sequences_cpu.py share: long-lived modules, train steps and evaluators under
MIXED call sequences -- batch sizes 4, 6, 1, 4 on one object, train / eval interleaved, policies changed, eager steps after a capture.

The property is HISTORY INDEPENDENCE: the result of call k on a long-lived object A depends on parameters, buffers, optimiser state, inputs
and policy only -- not on the shapes, modes, slots or policies A served before.  The truth for call k is a FRESH TWIN: new modules and a
new step / evaluator (`fresh_twin`), loaded from a `snapshot` of A taken just before the call (state_dict after flush_counters, Adam's m /
v / step), making the same one call.  `same_bits` compares with torch.equal: the suite already holds whole trajectories bitwise equal
between replicas and between eager and replayed steps, so no tolerance appears here.

The builders are those of the existing GPU tests (imported, their module-level DEV pointed at the device asked for: the dry-run script of
the CPU file asks for "cpu").  One call is a tuple (kind, N, data seed); `run_call` makes it on A or on a twin."""
import zlib

import torch

from oracle import tpgsr_oracle as O

BATCHES = (4, 6, 1, 4)      # 4: a plan to come back to; 6: regrows the shared scratch, other wgrad splits; 1: the smallest batch; 4: the plan
                            # recorded before its scratch was replaced
ADAM_KEYS = ("m", "v", "step")


# ---- builders --------------------------------------------------------------------------------------------------------------------------
def _from(module_name, dev):
    import importlib
    mod = importlib.import_module(module_name)
    mod.DEV = dev
    return mod


def build_tsrn(dev, stn=False):
    """the network of tests/test_fullsize_gpu.py test_module_api_two_forwards_before_backward (built inline there), with or without the STN head"""
    from tpgsr_amd.model import tsrn
    sd = O.recipe_state_dict(O.tsrn_spec(STN=stn, mask=True, srb_nums=2), 77, tps_hw=(16, 64) if stn else None)
    net = tsrn.TSRN(STN=stn, mask=True, srb_nums=2)
    net.load_state_dict(sd)
    return net.to(dev)


def build_tsrn_tl(dev):
    return _from("test_tsrn_gpu", dev)._build_tl(stn=False)[0]


def build_crnn(dev):
    return _from("test_crnn_gpu", dev)._build()[0]


def build_srres(dev):
    return _from("test_plain_baselines_gpu", dev).load("srres")


def build_edsr(dev):
    return _from("test_edsr_gpu", dev).load(2, 2)


def build_rrdb(dev):
    return _from("test_rrdb_gpu", dev).load(2, 2)


def _lr(N, seed, dev):
    return O.synthetic_batch(N, seed)[0].to(dev)


def _prior(N, seed, dev):
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.softmax(torch.randn(N, 37, 1, 26, generator=g), 1).to(dev)


# name -> (builder(dev) -> module, inputs(N, seed, dev) -> the module's arguments)
MODULES = {
    "tsrn": (build_tsrn, lambda N, s, dev: (_lr(N, s, dev),)),
    "tsrn_stn": (lambda dev: build_tsrn(dev, True), lambda N, s, dev: (_lr(N, s, dev),)),
    "tsrn_tl": (build_tsrn_tl, lambda N, s, dev: (_lr(N, s, dev), _prior(N, s, dev))),
    "crnn": (build_crnn, lambda N, s, dev: (O.parse_crnn_data(O.synthetic_batch(N, s)[0]).to(dev),)),
    "srres": (build_srres, lambda N, s, dev: (_lr(N, s, dev),)),
    "edsr": (build_edsr, lambda N, s, dev: (_lr(N, s, dev)[:, :3].contiguous(),)),
    "rrdb": (build_rrdb, lambda N, s, dev: (_lr(N, s, dev)[:, :3].contiguous(),)),
}


class Mods(list):
    """a list of modules that knows which row of MODULES it was built from"""
    kind = None


def module_builder(name, dev, training=False):
    """-> builder() of a one-module list (what snapshot / fresh_twin take for the module API)"""
    def build():
        mods = Mods([MODULES[name][0](dev).train(training)])
        mods.kind = name
        return mods
    return build


def step_builder(name, dev, precision=None):
    """-> builder() of a single-network train step: TSRNTrainStep on TSRN (with and without the STN head); SRTrainStep on srres (running
    statistics, _pending_batches of a functional engine), EDSR / RRDBNet with channels=3 (lr_c / hr_c in the static set)"""
    def build():
        from tpgsr_amd.interfaces.super_resolution import SRTrainStep, TSRNTrainStep
        net = MODULES[name][0](dev).train()
        if name in ("tsrn", "tsrn_stn"):
            ts = TSRNTrainStep(net, precision=precision)
        elif name == "srres":
            ts = SRTrainStep(net, image_crit="mse", precision=precision)
        else:
            ts = SRTrainStep(net, image_crit="l1", channels=3, precision=precision)
        ts.kind = name
        return ts
    return build


def cascade_builder(dev, stu_iter=1, precision=None):
    """-> builder() of the C3 cascade of tests/test_crnn_gpu.py (stu_iter 2: one shared SR network, a student per stage, so the SR engine's
    slots 0 and 1 are reused by every step) with a long-lived TextSREvaluator over the same modules, the teacher as its recogniser"""
    def build():
        from tpgsr_amd.interfaces.super_resolution import TextSREvaluator, TPGSRTrainStep
        srs, stus, teacher, *_ = _from("test_crnn_gpu", dev)._c3_models(n_stu=stu_iter)
        ts = TPGSRTrainStep(srs, stus, teacher, stu_iter=stu_iter, sr_share=True, precision=precision)
        ts.ev = TextSREvaluator(srs, stus, recognizer=teacher, stu_iter=stu_iter, sr_share=True)
        ts.kind = "cascade"
        return ts
    return build


# ---- the sequence tables: (kind, N, data seed) --------------------------------------------------------------------------------------------
EVAL_SEQ = [("eval", N, 10 + k) for k, N in enumerate(BATCHES)]
# train steps at 4, 6, 1, 4 with an eval forward at N = 6 on the same module between them (eval(), then train() again)
STEP_SEQ = [("step", 4, 20), ("eval", 6, 21), ("step", 6, 22), ("eval", 6, 23), ("step", 1, 24), ("eval", 6, 25), ("step", 4, 26)]
# the cascade: steps at 4, 6, 4, an evaluator batch at N = 6 and at N = 1 between them
CASCADE_SEQ = [("step", 4, 30), ("evb", 6, 31), ("step", 6, 32), ("evb", 1, 33), ("step", 4, 34)]
# capture at N = 4, replay, an eager step at N = 6 (the ragged last batch), replay with new N = 4 data, an eager step at N = 4
CAPTURE_SEQ = [("capture", 4, 40), ("replay", 4, 41), ("step", 6, 42), ("replay", 4, 43), ("step", 4, 44)]
POLICIES = ("f32", "x2", "x3", "bf16", "f32")


def training_only(seq):
    return [op for op in seq if op[0] == "step"]


def twin_op(op):
    """what a fresh twin does for call `op`: a capture (warm-up 1: ONE eager step, the capture itself executes nothing) and a replay are an
    eager step of the twin -- the suite holds replayed and eager steps bitwise equal"""
    return ("step",) + tuple(op[1:]) if op[0] in ("capture", "replay") else op


# ---- snapshot / twin / comparison -----------------------------------------------------------------------------------------------------
def modules_of(obj):
    if hasattr(obj, "pool"):
        return list(obj.pool.modules) + list(obj.frozen)
    return list(obj)


def snapshot(obj):
    """obj: a train step or a list of modules -> every module's state_dict (after flush_counters) and mode, and for a step Adam's m, v, step"""
    mods = modules_of(obj)
    for m in mods:
        m._engine().flush_counters()
    snap = dict(sd=[{k: v.detach().clone() for k, v in m.state_dict().items()} for m in mods], training=[m.training for m in mods], adam=None)
    if hasattr(obj, "opt"):
        snap["adam"] = [{k: obj.opt.state[id(m)][k].clone() for k in ADAM_KEYS} if id(m) in obj.opt.state else None for m in obj.pool.modules]
    return snap


def fresh_twin(snap, builder):
    """new modules and a new step / evaluator from `builder()`, loaded from the snapshot"""
    obj = builder()
    mods = modules_of(obj)
    assert len(mods) == len(snap["sd"])
    for m, sd, training in zip(mods, snap["sd"], snap["training"]):
        m.load_state_dict(sd, strict=True)
        m.train(training)
    if snap["adam"] is not None:
        obj._bind(next(mods[0].parameters()).device)
        for m, st in zip(obj.pool.modules, snap["adam"]):
            if st is not None:
                mine = obj.opt._st(m)[1]
                for k in ADAM_KEYS:
                    mine[k].copy_(st[k])
    return obj


def state_bits(obj, grads=True):
    """everything a call may leave behind: buffers (num_batches_tracked after a flush), the parameter arenas, and -- unless the call was an
    evaluation, which writes no gradient (a twin's gradient arena is still zero then) -- the gradient arenas; for a step Adam's m, v, step"""
    out = {}
    mods = modules_of(obj)
    for i, m in enumerate(mods):
        m._engine().flush_counters()
        for k, b in m.named_buffers():
            out[f"buffer{i}.{k}"] = b
    if hasattr(obj, "pool"):
        out["pool.flat"] = obj.pool.flat
        if grads:
            out["pool.grad"] = obj.pool.grad
        for i, m in enumerate(obj.pool.modules):
            st = obj.opt.state.get(id(m))
            for k in ADAM_KEYS if st is not None else ():
                out[f"adam{i}.{k}"] = st[k]
        for i, m in enumerate(obj.frozen):
            out[f"frozen{i}.flat"] = m._engine().arena.flat
    else:
        for i, m in enumerate(mods):
            a = m._engine().arena
            if a.flat is not None:
                out[f"arena{i}.flat"] = a.flat
                if grads:
                    out[f"arena{i}.grad"] = a.grad
    return out


def same_bits(a, b, tag):
    """a, b: dicts of tensors / plain values -> bitwise equal, or an AssertionError naming the first differing key and flat index"""
    assert sorted(a) == sorted(b), (tag, sorted(set(a) ^ set(b)))
    for k in a:
        x, y = a[k], b[k]
        if not isinstance(x, torch.Tensor):
            assert x == y, f"{tag}: {k}: {x!r} != {y!r}"
            continue
        assert x.shape == y.shape and x.dtype == y.dtype, f"{tag}: {k}: {tuple(x.shape)} {x.dtype} against {tuple(y.shape)} {y.dtype}"
        if torch.equal(x, y):
            continue
        xf, yf = x.detach().reshape(-1).cpu(), y.detach().reshape(-1).cpu()
        idx = (xf != yf).nonzero().reshape(-1)
        i = int(idx[0])
        msg = f"{tag}: {k} differs at flat index {i} ({idx.numel()} of {xf.numel()} elements): {xf[i].item()!r} against {yf[i].item()!r}"
        print(msg)
        raise AssertionError(msg)


def _value(v):
    return v.detach().clone() if isinstance(v, torch.Tensor) else v


def run_call(obj, op, dev, held=None):
    """make call `op` on `obj` -> what it returned, cloned (dict).  held: a list that receives (tag, the returned tensor itself, its clone)
    for the aliasing check at the end of a sequence (`check_held`).  The loss scalar of step() / replay() is a documented static buffer of
    the step (rewritten by the next step at that shape) and `last_sr` of a replay lives in the captured graph's pool: both are exempt."""
    kind, N, seed = op
    out, keep = {}, {}
    if kind == "eval":
        step = hasattr(obj, "pool")
        net = obj.model if step else obj[0]
        args = MODULES[obj.kind][1](N, seed, dev)
        was = net.training
        net.eval()
        try:
            with torch.no_grad():
                keep["y"] = net(*args)
        finally:
            net.train(was)
    elif kind == "step":
        lr, hr = [t.to(dev) for t in O.synthetic_batch(N, seed)]
        out["loss"] = _value(obj.step(lr, hr))
        keep["last_sr"] = obj.last_sr
        if hasattr(obj, "last_p"):
            out["last_p"] = _value(obj.last_p)
    elif kind == "capture":
        lr, hr = [t.to(dev) for t in O.synthetic_batch(N, seed)]
        obj.capture(lr, hr, warmup=1)
        out["loss"] = _value(obj._graph_loss)      # (the capture executed nothing: the static scalar still holds the warm-up step's loss)
    elif kind == "replay":
        lr, hr = [t.to(dev) for t in O.synthetic_batch(N, seed)]
        out["loss"] = _value(obj.replay(lr, hr))
        out["last_sr"] = _value(obj.last_sr)
        if hasattr(obj, "last_p"):
            out["last_p"] = _value(obj.last_p)
    elif kind == "evb":
        lr, hr = [t.to(dev) for t in O.synthetic_batch(N, seed)]
        mods = obj.pool.modules
        for m in mods:
            m.eval()
        try:
            from tpgsr_amd import kernels as K
            if K.DRYRUN:      # nothing is computed, so no strings or metrics can be made of the images: the launches up to them are traced
                srs, priors = obj.ev.super_resolve(lr)
                obj.ev.recognizer._engine().forward(torch.empty(N, 1, 32, 100), False)
                res = dict(images_sr=srs, priors=priors, psnr=0.0, ssim=0.0, pred_sr=[], pred_lr=[], pred_hr=[])
            else:
                res = obj.ev.eval_batch(lr, hr)
        finally:
            for m in mods:
                m.train()
        for i, t in enumerate(res["images_sr"]):
            keep[f"sr{i}"] = t
        for i, t in enumerate(res["priors"]):
            keep[f"prior{i}"] = t
        out.update(psnr=_value(res["psnr"]), ssim=_value(res["ssim"]), pred_sr=list(res["pred_sr"]), pred_lr=list(res["pred_lr"]),
                   pred_hr=list(res["pred_hr"]))
    else:
        raise ValueError(kind)
    for k, t in keep.items():
        out[k] = _value(t)
        if held is not None:
            held.append((f"{op} {k}", t, out[k]))
    return out


def check_held(held):
    """outputs are not aliased: every tensor a call returned earlier in the sequence still equals the clone taken when it was returned"""
    for tag, t, clone in held:
        assert torch.equal(t, clone), f"{tag}: a later call overwrote this returned tensor"


def run_sequence(builder, seq, dev, compare, grads_after=("step", "capture", "replay")):
    """the long-lived object A through `seq`; before every call a snapshot, after it `compare(k, op, A, out_A, twin, out_twin)` with a fresh
    twin that made the same call.  -> A"""
    A = builder()
    held = []
    for k, op in enumerate(seq):
        snap = snapshot(A)
        out_a = run_call(A, op, dev, held)
        B = fresh_twin(snap, builder)
        out_b = run_call(B, twin_op(op), dev)
        compare(k, op, A, out_a, B, out_b)
    check_held(held)
    return A


# ---- launch trace (dry run): names and non-pointer arguments ----------------------------------------------------------------------------
def install_trace():
    """-> the list every launch made outside a recording ("launch <entry point> <crc of its scalar arguments>") and every Plan.run ("plan
    <name> <ops> <crc over its ops' names, streams and scalar arguments>") is appended to, in order (tests/test_step_trace_cpu.py's spy,
    plus the plan's content: a replayed plan's geometry is part of what a call launches)"""
    from plan_signature import fields
    from tpgsr_amd import _lib, kernels as K
    lines = []
    launch, run = K._launch, K.Plan.run

    def scalars(fn, args):
        vals = []
        for t, a in zip(fn.argtypes, args):
            if t in (_lib.ci, _lib.ll, _lib.cf):
                vals.append(round(float(a), 6))
            elif t is not _lib.vp:
                fields(a._obj, vals)
        return vals

    def launch_spy(name, *args):
        if K._REC is None:
            lines.append("launch %s %08x" % (name, zlib.crc32(repr(scalars(getattr(_lib.load(), name), args)).encode())))
        return launch(name, *args)

    def run_spy(plan):
        sig = [(name, sid, args if fn is None else scalars(fn, args)) for name, fn, args, sid in plan.ops]
        lines.append("plan %s %d %08x" % (plan.name, len(plan.ops), zlib.crc32(repr(sig).encode())))
        return run(plan)

    K._launch, K.Plan.run = launch_spy, run_spy
    return lines
