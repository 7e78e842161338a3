"""CPU: the C-ABI shared library loads and exports every symbol include/tpgsr_hip.h declares, and the ctypes binding derived from that
header (tpgsr_amd/_abi.py, _lib.py) states what the C++ compiler reads in it (no kernel is launched)."""
import ctypes
import keyword
import os
import re
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def lib():
    from tpgsr_amd import build
    path = build.build()
    import torch  # noqa: F401  (HIP runtime load order, see tpgsr_amd/_lib.py)
    return ctypes.CDLL(path)


def declared_symbols():
    hdr = open(os.path.join(ROOT, "include", "tpgsr_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(tpgsr_[a-z0-9_]+)\s*\(", hdr)))


def test_header_symbols_exported(lib):
    names = declared_symbols()
    assert len(names) >= 40
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing


def test_release_build_has_no_lab_switches(lib):
    """the kernels' debug switches (parts of a kernel switched off for timing: results are garbage with any bit set) exist in LAB builds only
    (-DTPGSR_LAB, tools/lab/*_probe.py): a release library neither exports them nor declares them"""
    if os.environ.get("TPGSR_LAB"):
        pytest.skip("this IS a lab build")
    for name in ("tpgsr_wgh_debug", "tpgsr_gp_debug", "tpgsr_gru_debug"):
        assert not hasattr(lib, name), f"{name} is exported by a release build"
        assert name not in declared_symbols()


def test_binding_table_matches_header():
    from tpgsr_amd import _lib
    assert sorted(_lib.EXPORTED_SYMBOLS) == declared_symbols()


def test_struct_layouts(lib):
    from tpgsr_amd import _lib
    lib.tpgsr_sizeof.restype = ctypes.c_int
    for which, st in enumerate(_lib.ABI_STRUCTS):
        assert lib.tpgsr_sizeof(which) == ctypes.sizeof(st), st.__name__
    assert len(_lib.ABI_STRUCTS) == 13 and lib.tpgsr_sizeof(13) == -1    # the list covers every struct the library knows
    assert set(_lib.ABI_STRUCTS) == set(_lib._CLASSES.values()) and set(_lib._CLASSES) == set(_lib.ABI.structs)  # ... and every struct / union the header declares


_CXX = {ctypes.c_int: "int", ctypes.c_longlong: "long long", ctypes.c_ulonglong: "unsigned long long", ctypes.c_float: "float",
        ctypes.c_double: "double", ctypes.c_char_p: "const char*", None: "void"}
_PRELUDE = """#include <cstddef>
#include <tuple>
#include <type_traits>
#include "%s"
template <class F> struct sig;
template <class R, class... A> struct sig<R (*)(A...)> {
  using ret = R;
  static constexpr int arity = sizeof...(A);
  template <int i> using arg = std::tuple_element_t<i, std::tuple<A...>>;
};
template <class P> using pointee = std::remove_cv_t<std::remove_pointer_t<P>>;
#define SAME(...) static_assert(std::is_same<__VA_ARGS__>::value, #__VA_ARGS__)
#define PTR(...) static_assert(std::is_pointer<__VA_ARGS__>::value, #__VA_ARGS__)
"""


def binding_facts(sigs, structs):
    """One static_assert per fact of a binding -- sigs {symbol: (restype, [argtypes])}, structs {C name: ctypes class} -- in a C++ unit
    that includes the header: size of every struct, offset / size / type of every field, arity of every function, every scalar parameter
    and return type exactly, every pointer parameter a pointer, to the very struct where the binding types it"""
    from tpgsr_amd import _lib
    cname = {cls: c for c, cls in list(_lib._CLASSES.items()) + list(structs.items())}

    def typed(expr, t):
        if t in _CXX:
            return [f"SAME({expr}, {_CXX[t]});"]
        if t in cname:                                                             # a nested struct, by value
            return [f"SAME({expr}, {cname[t]});"]
        if t is ctypes.c_void_p:
            return [f"PTR({expr});"]
        return [f"PTR({expr});", f"SAME(pointee<{expr}>, {cname[t._type_]});"]      # POINTER(struct)

    out = [_PRELUDE % os.path.join(ROOT, "include", "tpgsr_hip.h")]
    for c, cls in structs.items():
        out.append(f"static_assert(sizeof({c}) == {ctypes.sizeof(cls)}, \"sizeof {c}\");")
        for name, t in cls._fields_:
            f, d = name[:-1] if name.endswith("_") and keyword.iskeyword(name[:-1]) else name, getattr(cls, name)
            out.append(f"static_assert(offsetof({c}, {f}) == {d.offset} && sizeof({c}::{f}) == {d.size}, \"{c}.{f}\");")
            out += typed(f"decltype({c}::{f})", t)
    for name, (res, args) in sigs.items():
        out.append(f"static_assert(sig<decltype(&{name})>::arity == {len(args)}, \"arity of {name}\");")
        out += typed(f"sig<decltype(&{name})>::ret", res)
        for i, t in enumerate(args):
            out += typed(f"sig<decltype(&{name})>::arg<{i}>", t)
    return "\n".join(out) + "\n"


def compiles(unit, tmp_path):
    """host-only syntax check by the compiler that builds the library: no device code, no linking, no GPU"""
    from tpgsr_amd import build
    src = tmp_path / "abi_facts.cpp"
    src.write_text(unit)
    r = subprocess.run([build._hipcc(), "-x", "c++", "-std=c++17", "-fsyntax-only", str(src)], capture_output=True, text=True)
    return r.returncode == 0, r.stdout + r.stderr


def derived_binding():
    from tpgsr_amd import _lib
    return dict(_lib._SIGS), dict(_lib._CLASSES)


def test_derived_binding_is_what_the_compiler_reads(tmp_path):
    sigs, structs = derived_binding()
    assert len(sigs) >= 150 and len(structs) == 13
    unit = binding_facts(sigs, structs)
    assert unit.count("static_assert") + unit.count("SAME(") + unit.count("PTR(") > 1400
    ok, log = compiles(unit, tmp_path)
    assert ok, log


def test_compiler_check_catches_a_wrong_width(tmp_path):
    """mutant: `long long count` of tpgsr_bn_finalize transcribed as int -- same name, same arity, truncates on the GPU"""
    sigs, structs = derived_binding()
    res, args = sigs["tpgsr_bn_finalize"]
    assert args[3] is ctypes.c_longlong
    sigs["tpgsr_bn_finalize"] = (res, args[:3] + [ctypes.c_int] + args[4:])
    ok, log = compiles(binding_facts(sigs, structs), tmp_path)
    assert not ok and "tpgsr_bn_finalize" in log and "arg<3>" in log, log


def test_compiler_check_catches_swapped_fields(tmp_path):
    """mutant: two adjacent int fields of tpgsr_conv_route_t swapped -- sizeof, all that was compared before, does not change"""
    sigs, structs = derived_binding()
    fields = list(structs["tpgsr_conv_route_t"]._fields_)
    i = [f for f, _ in fields].index("lcap")
    assert fields[i][1] is fields[i + 1][1] is ctypes.c_int
    fields[i], fields[i + 1] = fields[i + 1], fields[i]
    mutant = type("ConvRoute", (ctypes.Structure,), {"_fields_": fields})
    assert ctypes.sizeof(mutant) == ctypes.sizeof(structs["tpgsr_conv_route_t"])
    structs["tpgsr_conv_route_t"] = mutant
    ok, log = compiles(binding_facts(sigs, structs), tmp_path)
    assert not ok and "tpgsr_conv_route_t.lcap" in log and "tpgsr_conv_route_t.nbw" in log, log


SNIPPET = """
#ifndef X_H
#define X_H
#ifdef __cplusplus
extern "C" {
#endif
#define X_ON 1   /* a constant */
#define X_OFF -2
enum x_kind { X_A = 0, X_B = 1, X_C };
typedef struct {
  const float *in, *in2;     /* pointer attached to the name */
  float* out;                /* ... and to the type */
  int N, H,
      W;
  unsigned long long seed;
} x_args;
typedef struct x_outer { x_args a; double f; const x_args* next; } x_outer;
typedef union x_val { const void* p; long long i; } x_val;
int x_run(const x_args* a, const x_outer *o,
          long long n, unsigned long long seed, void* stream);
int x_table(const x_args* items_dev, int* const* steps, const unsigned int* mask);
const char* x_name(void);
void x_set(int on);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_header_reader_on_snippets():
    from tpgsr_amd import _abi
    h = _abi.parse(SNIPPET)
    assert h.defines == {"X_ON": 1, "X_OFF": -2}
    assert h.enums == {"x_kind": [("X_A", 0), ("X_B", 1), ("X_C", 2)]}
    assert list(h.structs) == ["x_args", "x_outer", "x_val"]                        # declaration order
    assert h.structs["x_args"] == ("struct", [("in", "const float*"), ("in2", "const float*"), ("out", "float*"), ("N", "int"), ("H", "int"),
                                              ("W", "int"), ("seed", "unsigned long long")])
    assert h.structs["x_outer"] == ("struct", [("a", "x_args"), ("f", "double"), ("next", "const x_args*")])     # nested, by name
    assert h.structs["x_val"] == ("union", [("p", "const void*"), ("i", "long long")])
    assert h.functions["x_run"] == ("int", [("const x_args*", "a"), ("const x_outer*", "o"), ("long long", "n"),
                                            ("unsigned long long", "seed"), ("void*", "stream")])                # wrapped over two lines
    assert h.functions["x_table"] == ("int", [("const x_args*", "items_dev"), ("int* const*", "steps"), ("const unsigned int*", "mask")])
    assert h.functions["x_name"] == ("const char*", []) and h.functions["x_set"] == ("void", [("int", "on")])
    assert list(h.functions) == ["x_run", "x_table", "x_name", "x_set"]


@pytest.mark.parametrize("bad", ["int x_cb(void (*fn)(int), void* stream);", "int x_arr(const int dims[4]);", "typedef struct { int a : 3; } x_bits;",
                                 "typedef struct { int v[4]; } x_vec;", "size_t x_bytes(void);", "int x_old();", "int x_unnamed(int, float);",
                                 "typedef int x_int;", "static const int x_k = 3;", "#define X_F 1.5f", "#include <stddef.h>",
                                 "typedef struct { struct x_in { int a; } in; } x_nest;", "int x_run(const x_other* a);",
                                 "enum x_e { X_Q = 1 << 2 };", "int x_dup(int a); int x_dup(int a);"])
def test_header_reader_raises_on_what_it_cannot_read(bad):
    """a declaration outside the subset fails loudly and is named: it must never drop out of the binding silently"""
    from tpgsr_amd import _abi
    good = "int x_before(int a);\n%s\nint x_after(int b);\n"
    assert list(_abi.parse(good % "").functions) == ["x_before", "x_after"]
    with pytest.raises(_abi.HeaderError) as e:
        _abi.parse(good % bad)
    named = re.findall(r"x_\w+|X_\w+|stddef", bad)[0]
    assert named in str(e.value), str(e.value)


def test_type_mapping_of_the_binding():
    """the header's conventions as ctypes: struct pointers typed, device-resident tables (`*_dev`) and every other pointer an address"""
    from tpgsr_amd import _lib
    P, vp, ci, ll = ctypes.POINTER, ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    S = _lib._SIGS
    assert S["tpgsr_conv_fwd"] == (ci, [P(_lib.ConvArgs), vp])
    assert S["tpgsr_conv_wgrad_batch"] == (ci, [vp, ci, ci, ci, ci, vp])                       # items_dev
    assert S["tpgsr_conv_wgrad_batch_prepare"] == (ci, [P(_lib.WgradArgs), P(_lib.WgradBatchItem)])
    assert S["tpgsr_resize_normalize"][1][:3] == [vp, vp, vp]                                  # pixels, descs_dev, tables_dev
    assert S["tpgsr_wgrad_halo_plan"] == (ci, [P(_lib.ConvArgs), vp, vp])
    assert S["tpgsr_plan_set_mode"] == (None, [ci, ci, ctypes.c_ulonglong, ci])
    assert S["tpgsr_lstm_seq_hx_bytes"] == (ll, []) and S["tpgsr_last_error"] == (ctypes.c_char_p, [])
    assert S["tpgsr_plan_create"] == (vp, []) and S["tpgsr_plan_add_launch"][1] == [vp, ctypes.c_char_p, P(_lib.PlanArg), ci, ci]
    assert S["tpgsr_bn_finalize"][1][3] is ll and S["tpgsr_add"][1][2] is ll
    assert _lib.ConvArgs._fields_[0] == ("in_", vp) and _lib.WgradArgs._fields_[0] == ("c", _lib.ConvArgs)
    assert issubclass(_lib.PlanArg, ctypes.Union) and _lib.PlanArg._fields_ == [("p", vp), ("i", ll), ("f", ctypes.c_double)]
    assert _lib.CONV_KERNELS[5] == "xbf_halo3" and _lib.WGRAD_KERNELS[4] == "xbf_3k" and len(_lib.CONV_KERNELS) == 9
    assert (_lib.ACT_NONE, _lib.ACT_RELU, _lib.ACT_MISH, _lib.ACT_TANH, _lib.ACT_PRELU) == (0, 1, 2, 3, 4)
    for arg in (ctypes.byref(ll()), (ctypes.c_float * 2)(), ctypes.pointer(ci()), 0x1000, None):  # what callers hand to an address parameter
        vp.from_param(arg)


def test_error_reporting_without_gpu(lib):
    lib.tpgsr_last_error.restype = ctypes.c_char_p
    lib.tpgsr_conv_fwd.restype = ctypes.c_int
    rc = lib.tpgsr_conv_fwd(None, None)          # rejected before any launch
    assert rc == -1 and b"null" in lib.tpgsr_last_error()
    assert lib.tpgsr_version() >= 1


def test_conv_rejects_operands_past_the_buffer_window(lib):
    """the conv loaders address operands with 32-bit byte offsets in a 2 GiB window: a bigger operand is rejected before any
    launch instead of being read as zeros"""
    from tpgsr_amd import _lib
    lib.tpgsr_last_error.restype = ctypes.c_char_p
    a = _lib.ConvArgs()
    a.in_ = 0x1000
    a.wt = 0x2000
    a.out = 0x3000
    a.N, a.H, a.W, a.Cin, a.in_ld = 4096, 32, 128, 64, 64            # 4 GiB of fp32 activations
    a.Cout, a.KH, a.KW, a.pad_h, a.pad_w, a.OH, a.OW, a.out_ld = 64, 3, 3, 1, 1, 32, 128, 64
    rc = lib.tpgsr_conv_fwd(ctypes.byref(a), None)
    assert rc == -1 and b"2 GiB" in lib.tpgsr_last_error()
    a.N = 1024                                                        # 1 GiB input, but a dy of 1024 x 4096 x 640 floats
    w = _lib.WgradArgs()
    w.c = a
    w.dy, w.part, w.dy_ld = 0x4000, 0x5000, 640
    rc = lib.tpgsr_conv_wgrad(ctypes.byref(w), None)
    assert rc == -1 and b"2 GiB" in lib.tpgsr_last_error()


def test_product_path_has_no_cpu_fallback():
    import torch
    from tpgsr_amd.model import tsrn
    net = tsrn.TSRN(STN=False, mask=True)
    with pytest.raises(RuntimeError, match="no CPU"):
        net(torch.zeros(1, 4, 16, 64))
    # the product package never imports the oracle
    import subprocess
    import sys
    out = subprocess.run([sys.executable, "-c", "import sys, tpgsr_amd.engine, tpgsr_amd.interfaces.super_resolution, "
                          "tpgsr_amd.loss.image_loss; print(any(m.startswith('oracle') for m in sys.modules))"],
                         capture_output=True, text=True, cwd=ROOT)
    assert out.stdout.strip() == "False", out.stdout + out.stderr


def test_native_plan_records_without_gpu():
    """The plan executor (csrc/plan.cpp) can be built, inspected and rejected arguments reported with no device."""
    from tpgsr_amd import _lib
    lib = _lib.load()
    h = lib.tpgsr_plan_create()
    try:
        args = (_lib.PlanArg * 4)()
        args[0].p, args[1].p, args[2].i, args[3].p = 0x1000, 0x2000, 16, 0x3000
        assert lib.tpgsr_plan_add_launch(h, b"tpgsr_add", args, 4, 0) == 0
        assert lib.tpgsr_plan_add_fork(h) == 1
        ca = _lib.ConvArgs()
        one = (_lib.PlanArg * 1)()
        one[0].p = ctypes.addressof(ca)
        assert lib.tpgsr_plan_add_launch(h, b"tpgsr_conv_fwd", one, 1, 1) == 2
        assert lib.tpgsr_plan_add_join(h) == 3
        assert lib.tpgsr_plan_size(h) == 4
        v = _lib.PlanArg()
        v.p = 0x4000
        assert lib.tpgsr_plan_set_arg(h, 0, 3, ctypes.byref(v)) == 0
        assert lib.tpgsr_plan_set_arg(h, 2, 0, ctypes.byref(v)) < 0          # the copied argument struct is not patchable
        assert lib.tpgsr_plan_add_launch(h, b"tpgsr_add", args, 3, 0) < 0     # wrong arity
        assert b"arguments" in lib.tpgsr_last_error()
        assert lib.tpgsr_plan_add_launch(h, b"tpgsr_version", args, 0, 0) < 0  # not a launch entry point
        assert lib.tpgsr_plan_size(h) == 4
    finally:
        lib.tpgsr_plan_destroy(h)


def test_cu_mask_spec_parsing():
    from tpgsr_amd import kernels as K
    assert K.parse_cu_mask("0xff") == [0xFF]
    assert K.parse_cu_mask("40") == [0xFFFFFFFF, 0xFF]
    assert K.parse_cu_mask("4/16") == [0x00010001, 0x00010001]
    assert K.parse_cu_mask("0x1" + "0" * 16) == [0, 0, 1]


def test_plan_recording_sections_on_cpu():
    """Plan bookkeeping without a device: side sections tag launches, fork/join edges are emitted once per section / plan,
    DynPtr slots are tracked, and the native handle is built lazily (not here)."""
    from tpgsr_amd import kernels as K
    plan = K.Plan("t")
    plan.overlap = True
    with K.recording(plan):
        K._launch("tpgsr_zero", 0x1000, 16)
        with K.side():
            K._launch("tpgsr_zero", K.DynPtr("buf"), 16)
            K._launch("tpgsr_zero", 0x3000, 16)
        K._launch("tpgsr_zero", 0x4000, 16)
        plan.join()
        plan.join()                                   # idempotent: nothing to join any more
    kinds = [(op[0], op[3]) for op in plan.ops]
    assert kinds == [("tpgsr_zero", 0), ("fork", 0), ("tpgsr_zero", 1), ("tpgsr_zero", 1), ("tpgsr_zero", 0), ("join", 0)]
    assert plan.dyn == {"buf": [(2, 0)]} and plan._native is None
    plan.set_ptr("buf", 0x2000)
    assert plan.ops[2][2][0] == 0x2000
    plain = K.Plan("p")                               # overlap off: side() is a no-op
    with K.recording(plain):
        with K.side():
            K._launch("tpgsr_zero", 0x1000, 16)
        plain.join()
    assert [(op[0], op[3]) for op in plain.ops] == [("tpgsr_zero", 0)]


def test_plan_side_batch_on_cpu():
    """side_batch_begin / _end: the side sections in between are held and go out behind ONE fork at the end of the batch, in order,
    DynPtr slots pointing at their final op index; the caller's launches keep their order"""
    from tpgsr_amd import kernels as K
    plan = K.Plan("b")
    plan.overlap = True
    with K.recording(plan):
        K._launch("tpgsr_zero", 0x1000, 16)
        sb = K.side_batch_begin()
        assert sb
        with K.side():
            K._launch("tpgsr_zero", 0x2000, 16)
        K._launch("tpgsr_zero", K.DynPtr("m"), 16)
        with K.side():
            K._launch("tpgsr_zero", K.DynPtr("s"), 16)
        K._launch("tpgsr_zero", 0x5000, 16)
        K.side_batch_end(sb)
        with K.side():                                  # outside a batch: its own fork, as before
            K._launch("tpgsr_zero", 0x6000, 16)
        plan.join()
    kinds = [(op[0], op[3], op[2][0] if op[1] else None) for op in plan.ops]
    assert kinds == [("tpgsr_zero", 0, 0x1000), ("tpgsr_zero", 0, None), ("tpgsr_zero", 0, 0x5000), ("fork", 0, None),
                     ("tpgsr_zero", 1, 0x2000), ("tpgsr_zero", 1, None), ("fork", 0, None), ("tpgsr_zero", 1, 0x6000), ("join", 0, None)]
    assert plan.dyn == {"m": [(1, 0)], "s": [(5, 0)]}
    empty = K.Plan("e")                                 # a batch without side sections leaves nothing behind
    empty.overlap = True
    with K.recording(empty):
        sb = K.side_batch_begin()
        K._launch("tpgsr_zero", 0x1000, 16)
        K.side_batch_end(sb)
        empty.join()
    assert [(op[0], op[3]) for op in empty.ops] == [("tpgsr_zero", 0)]


def test_plan_continue_in_on_cpu():
    """K.continue_in: a pass recorded as two plans (the caller regains control in between).  The first plan leaves its side-stream work
    pending -- no join -- and the second plan's join is emitted even when it has no side section of its own"""
    from tpgsr_amd import kernels as K
    a, b = K.Plan("a"), K.Plan("b")
    a.overlap = b.overlap = True
    with K.recording(a):
        K._launch("tpgsr_zero", 0x1000, 16)
        with K.side():
            K._launch("tpgsr_zero", 0x2000, 16)
        K.continue_in(b)
        K._launch("tpgsr_zero", 0x3000, 16)
        K._REC.join()
    assert [(op[0], op[3]) for op in a.ops] == [("tpgsr_zero", 0), ("fork", 0), ("tpgsr_zero", 1)]
    assert [(op[0], op[3]) for op in b.ops] == [("tpgsr_zero", 0), ("join", 0)]
    c, d = K.Plan("c"), K.Plan("d")                    # nothing pending: no join needed in the second plan
    with K.recording(c):
        K._launch("tpgsr_zero", 0x1000, 16)
        K.continue_in(d)
        K._launch("tpgsr_zero", 0x3000, 16)
        K._REC.join()
    assert [(op[0], op[3]) for op in d.ops] == [("tpgsr_zero", 0)]
    e, f = K.Plan("e"), K.Plan("f")                    # not from inside a side section / a side batch
    e.overlap = True
    with K.recording(e):
        sb = K.side_batch_begin()
        with pytest.raises(AssertionError):
            K.continue_in(f)
        K.side_batch_end(sb)
