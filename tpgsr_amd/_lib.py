"""ctypes binding of libtpgsr_hip.so (the C ABI declared in include/tpgsr_hip.h).

There is deliberately NO fallback: if the shared library is missing or a kernel call fails, the product path
raises.  The CPU oracle under oracle/ is test infrastructure and is never imported from here."""
import ctypes as C
import keyword
import os

# torch bundles its own HIP runtime (torch/lib/libamdhip64.so, soname libamdhip64.so.7).  It MUST be the one already
# mapped when libtpgsr_hip.so (NEEDED libamdhip64.so.7) is dlopen'ed, otherwise the process ends up with two HIP
# runtimes and every call on a torch stream fails with hipErrorNoDevice.  Importing torch first guarantees that.
import torch  # noqa: F401  (load-order dependency, see above)

from . import _abi  # noqa: E402

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libtpgsr_hip.so")

ABI = _abi.parse(open(os.path.join(_HERE, "..", "include", "tpgsr_hip.h")).read())   # the header csrc/*.cpp include, same relative place

vp = C.c_void_p
ci = C.c_int
ll = C.c_longlong
cf = C.c_float
_SCALARS = {"int": ci, "long long": ll, "unsigned long long": C.c_ulonglong, "float": cf, "double": C.c_double}

# The one hand-written list of the binding: Python class name of every argument struct / union of the header, in tpgsr_sizeof(which)
# order (csrc/error.cpp).  Fields, prototypes, enums and constants all come from the header itself.
_CLASS_NAMES = {"tpgsr_conv_args": "ConvArgs", "tpgsr_wgrad_args": "WgradArgs", "tpgsr_pack_desc": "PackDesc",
                "tpgsr_wgrad_reduce_desc": "WgradReduceDesc", "tpgsr_compose_bwd_desc": "ComposeBwdDesc", "tpgsr_split_desc": "SplitDesc",
                "tpgsr_image_desc": "ImageDesc", "tpgsr_gru_wgrad_args": "GruWgradArgs", "tpgsr_wgrad_batch_item": "WgradBatchItem",
                "tpgsr_bigru_proj_args": "BigruProjArgs", "tpgsr_conv_route_t": "ConvRoute", "tpgsr_wgrad_route_t": "WgradRoute",
                "tpgsr_plan_arg": "PlanArg"}
_CLASSES = {}


def _ctype(ctype, name=""):
    """ctypes type of a C type of the header.  Pointers are addresses (c_void_p: an integer, byref(), a ctypes array) except a pointer to
    an ABI struct, which is typed -- unless the parameter is a device-resident table (`*_dev`), whose address arrives as an integer."""
    if ctype == "const char*":
        return C.c_char_p
    if ctype.endswith("*"):
        cls = _CLASSES.get(ctype[:-1].replace("const ", ""))
        return C.POINTER(cls) if cls and not name.endswith("_dev") else vp
    if ctype in _CLASSES:
        return _CLASSES[ctype]
    if ctype not in _SCALARS:
        raise TypeError(f"include/tpgsr_hip.h: no ctypes mapping for {ctype!r} ({name})")
    return _SCALARS[ctype]


for _cname, (_kind, _fields) in ABI.structs.items():      # declaration order: a nested struct is built before its user
    _CLASSES[_cname] = type(_CLASS_NAMES[_cname], (C.Union if _kind == "union" else C.Structure,),
                            {"__doc__": _cname, "_fields_": [(f + "_" * keyword.iskeyword(f), _ctype(t, f)) for f, t in _fields]})
ABI_STRUCTS = tuple(_CLASSES[c] for c in _CLASS_NAMES)
globals().update({cls.__name__: cls for cls in ABI_STRUCTS})                                  # ConvArgs, WgradArgs, ..., PlanArg
globals().update({k[len("TPGSR_"):]: v for k, v in ABI.defines.items() if k.startswith("TPGSR_ACT_")})   # ACT_NONE, ..., ACT_PRELU
_ACT = {None: ACT_NONE, "none": ACT_NONE, "relu": ACT_RELU, "mish": ACT_MISH, "tanh": ACT_TANH}  # noqa: F821


def _kernel_names(enum, prefix):
    """TPGSR_CONV_XBF_HALO3 = 5 -> names[5] == "xbf_halo3": what tpgsr_conv_route_t.kernel indexes"""
    assert all(name.startswith(prefix) for name, _ in ABI.enums[enum]), enum
    names = {value: name[len(prefix):].lower() for name, value in ABI.enums[enum]}
    return tuple(names[i] for i in range(len(ABI.enums[enum])))      # KeyError: the values are not 0 .. n-1


CONV_KERNELS = _kernel_names("tpgsr_conv_kernel", "TPGSR_CONV_")
WGRAD_KERNELS = _kernel_names("tpgsr_wgrad_kernel", "TPGSR_WGRAD_")

_SIGS = {name: (None if ret == "void" else _ctype(ret), [_ctype(t, p) for t, p in params]) for name, (ret, params) in ABI.functions.items()}
EXPORTED_SYMBOLS = sorted(_SIGS)

_lib = None


class TpgsrKernelError(RuntimeError):
    pass


def load():
    """Load the shared library (building is __graft_entry__.build()'s / tpgsr_amd.build's job)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise TpgsrKernelError(
            f"{LIB_PATH} is missing: build it with `python -m tpgsr_amd.build` (hipcc --offload-arch=gfx950). "
            "tpgsr_amd has no CPU / PyTorch fallback by design.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    for which, st in enumerate(ABI_STRUCTS):
        if lib.tpgsr_sizeof(which) != C.sizeof(st):
            raise TpgsrKernelError(f"ABI mismatch: {st.__name__} is {C.sizeof(st)} bytes in the binding, "
                                   f"{lib.tpgsr_sizeof(which)} in {LIB_PATH}: rebuild (python -m tpgsr_amd.build)")
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().tpgsr_last_error().decode(errors="replace")
        raise TpgsrKernelError(f"{what or 'tpgsr kernel'} failed (rc={rc}): {msg}")


def act_code(name):
    return _ACT[name] if not isinstance(name, int) else name
