"""Reader of include/tpgsr_hip.h: the one declaration of the C ABI, from which _lib.py builds the ctypes binding.

It reads the C subset that header is written in and nothing more -- `#define NAME integer`, #ifdef / #ifndef / #endif, enums,
`typedef struct / union { fields } name;` (several declarators per field, ABI structs by value), prototypes -- and raises HeaderError,
quoting the text, on anything else: a declaration this reader does not understand must fail the import, not drop a symbol."""
import collections
import re

Header = collections.namedtuple("Header", "functions structs enums defines")
_SCALARS = ("unsigned long long", "long long", "unsigned char", "unsigned int", "unsigned", "int", "float", "double", "void", "char")


class HeaderError(ValueError):
    pass


def _preprocess(text, defines):
    """comments and directives out; an #ifdef / #ifndef block whose condition fails (`#ifdef __cplusplus`) goes with them"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    seen, taken, out = set(), [], []
    for line in text.split("\n"):
        if not line.lstrip().startswith("#"):
            out.append(line if all(taken) else "")
            continue
        word = line.replace("#", " ", 1).split() + [""]
        if word[0] in ("ifdef", "ifndef") and len(word) == 3:
            taken.append((word[1] in seen) == (word[0] == "ifdef"))
        elif word[0] == "endif" and len(word) == 2 and taken:
            taken.pop()
        elif not all(taken):
            pass
        elif word[0] == "define" and len(word) == 3:                               # the include guard
            seen.add(word[1])
        elif word[0] == "define" and len(word) == 4 and re.fullmatch(r"-?\d+", word[2]):
            seen.add(word[1])
            defines[word[1]] = int(word[2])
        else:
            raise HeaderError(f"unreadable preprocessor line: {line.strip()!r}")
    if taken:
        raise HeaderError("unbalanced #ifdef / #endif")
    return "\n".join(out)


# [const] base type, `*` / `* const` any number of times, name -- over text whose white space is single blanks
_DECLARATOR = re.compile(r"((?:const )?([A-Za-z_]\w*(?: [A-Za-z_]\w*)*?)) ?((?:\* ?(?:const\b ?)?)*)(\w+)")


def _declarator(text, structs, where, inherit=""):
    """`const float *in` -> ("const float*", "in", "const float"); the base type is a scalar or an ABI struct declared so far; `inherit`
    is the type part that a later declarator of a field list shares with the first"""
    m = _DECLARATOR.fullmatch(" ".join((inherit + " " + text).split()))
    if not m or (m.group(2) not in _SCALARS and m.group(2) not in structs) or m.group(4) in ("const",) + _SCALARS:
        raise HeaderError(f"unreadable declarator in {where}: {text.strip()!r}")
    return m.group(1) + m.group(3).replace(" ", "").replace("const", " const"), m.group(4), m.group(1)


def parse(text):
    """-> Header(functions {name: (return type, [(param type, param name)])}, structs {name: (kind, [(field name, type)])},
    enums {name: [(enumerator, value)]}, defines {NAME: integer}), every dict in declaration order"""
    h = Header({}, {}, {}, {})
    text = _preprocess(text, h.defines)
    top = re.compile(r"\s*(?:typedef\s+(struct|union)\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;|enum\s+(\w+)\s*\{([^{}]*)\}\s*;|([^;{}()]+)\(([^;{}()]*)\)\s*;)")
    pos = 0
    while text[pos:].strip():
        m = top.match(text, pos)
        if not m:
            raise HeaderError(f"unreadable declaration: {' '.join(text[pos:].split(';')[0].split())[:160]!r}")
        pos = m.end()
        kind, body, sname, ename, ebody, head, params = m.groups()
        if sname:
            fields = []
            for decl in filter(None, (d.strip() for d in body.split(";"))):
                first, *more = decl.split(",")
                ctype, name, base = _declarator(first, h.structs, sname)
                fields.append((name, ctype))
                for d in more:
                    ctype, name, _ = _declarator(d, h.structs, sname, base)
                    fields.append((name, ctype))
            if sname in h.structs or not fields or any(t == "void" for _, t in fields):
                raise HeaderError(f"unreadable {kind}: {sname}")
            h.structs[sname] = (kind, fields)
        elif ename:
            value, items = -1, []
            for item in filter(None, (i.strip() for i in ebody.split(","))):
                em = re.fullmatch(r"(\w+)(?:\s*=\s*(-?\d+))?", item)
                if not em:
                    raise HeaderError(f"unreadable enumerator of {ename}: {item!r}")
                value = value + 1 if em.group(2) is None else int(em.group(2))
                items.append((em.group(1), value))
            h.enums[ename] = items
        else:
            ret, fname, _ = _declarator(head, h.structs, "a prototype")
            plist = [] if params.strip() == "void" else [_declarator(p, h.structs, fname)[:2] for p in params.split(",")]
            if fname in h.functions or any(t == "void" for t, _ in plist):
                raise HeaderError(f"unreadable prototype: {fname}")
            h.functions[fname] = (ret, plist)
    return h
