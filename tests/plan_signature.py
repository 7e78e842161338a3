"""The plan signature of an engine (tests/test_hd64_cpu.py, tests/test_functional_plans_cpu.py; imported by their dry-run scripts): one
line per recorded op of every plan -- cache key, plan name, op name, stream id and a CRC of every integer / float the launch carries
(scalar arguments and the non-pointer fields of argument structs: the geometry the launcher derives its grid from).  "fork" / "join" /
"edge" ops are lines too.  Pointers are left out: they differ from run to run."""
import ctypes as C
import zlib

from tpgsr_amd import _lib
from tpgsr_amd.kernels import Plan

# the order the plans of one cache entry are listed in; any other Plan of the entry follows, sorted by its key
ORDER = ("pack", "pack_late", "pre", "fwd", "fwd_b", "bwd", "bwd_b", "dgray")


def fields(obj, out):
    for name, t in obj._fields_:
        v = getattr(obj, name)
        if isinstance(v, C.Structure):
            fields(v, out)
        elif t in (_lib.ci, _lib.ll, _lib.cf):
            out.append((name, round(float(v), 6)))


def signature(plans):
    """plans: an engine's `_plans` (cache key -> dict holding Plan values among its buffers)"""
    lines = []
    for key, pl in plans.items():
        names = [k for k in ORDER if isinstance(pl.get(k), Plan)] + sorted(k for k, v in pl.items() if isinstance(v, Plan) and k not in ORDER)
        for pname in names:
            plan = pl[pname]
            if len(plan):
                plan.run()                              # the native executor checks entry point and argument count
            for name, fn, args, sid in plan.ops:
                vals = []
                if fn is None:
                    vals.append(args)
                else:
                    for t, a in zip(fn.argtypes, args):
                        if t in (_lib.ci, _lib.ll, _lib.cf):
                            vals.append(round(float(a), 6))
                        elif t is not _lib.vp:
                            fields(a._obj, vals)
                crc = zlib.crc32(repr(vals).encode())
                lines.append("%s %s %s %d %08x" % ("/".join(str(k) for k in key), pname, name, sid, crc))
    return lines
