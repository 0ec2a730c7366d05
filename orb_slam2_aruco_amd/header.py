"""Reader of include/orbfe.h, the one statement of the C ABI: every ctypes prototype, record layout and integer constant the
Python plumbing uses is derived from it here, once per process, in pure Python (no compiler).

    functions   name -> (restype, [argtypes]) as ctypes types
    records     name -> [(field, scalar C type, array dimensions)]
    defines     every `#define ORBFE_<NAME> <integer>`, as "<NAME>" -> value

Parameters: any pointer or array is c_void_p (a `const char*` c_char_p), scalars map by SCALARS.  Returns: void is None,
`const char*` c_char_p, any other pointer c_void_p.  A declaration that does not fit (an unknown type, a function pointer, varargs,
a nested struct) raises HeaderError with its text; nothing is skipped, and the functions are counted against the header's
`orbfe_name(` occurrences."""
import ctypes as C
import os
import re

import numpy as np

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "orbfe.h")

SCALARS = {"char": C.c_char, "int": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t,
           "long long": C.c_longlong, "unsigned long long": C.c_ulonglong}
SCALARS.update({"%sint%d_t" % (u, b): getattr(C, "c_%sint%d" % (u, b)) for u in ("", "u") for b in (8, 16, 32, 64)})


class HeaderError(ValueError):
    pass


def _ctype(decl, pointees, param):
    """The ctypes type of a return type (param=False) or of one parameter with its name; `pointees`: what a pointer may point to."""
    words = re.sub(r"\b(const|struct)\b|\[\d*\]", " ", decl).replace("*", " ").split()
    if param:
        words = words[:-1]
    base, pointer = " ".join(words), "*" in decl or "[" in decl
    if not (base in SCALARS or (pointer and base in pointees)) or "(" in decl or "..." in decl:
        raise HeaderError("include/orbfe.h: cannot read the type of `%s`" % decl.strip())
    if not pointer:
        return SCALARS[base]
    return C.c_char_p if base == "char" and decl.count("*") == 1 and "[" not in decl else C.c_void_p


def _parse(text):
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    ncalls = len(re.findall(r"orbfe_\w+\s*\(", text))
    defines = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]*(.*)$", text, flags=re.M):
        m = re.fullmatch(r"\(?\s*(-?\w+)\s*\)?", value.strip())
        if name.startswith("ORBFE_") and value.strip():
            try:
                defines[name[6:]] = int(m.group(1), 0)
            except (AttributeError, ValueError):
                raise HeaderError("include/orbfe.h: #define %s %s is not an integer" % (name, value)) from None
    text = re.sub(r"#ifdef __cplusplus.*?#endif", " ", text, flags=re.S)     # extern "C" { and its }
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    records, record = {}, r"typedef\s+struct\s+\w+\s*\{([^{}]*)\}\s*(\w+)\s*;"
    for m in re.finditer(record, text):
        fields = records[m.group(2)] = []
        for decl in filter(None, (d.strip() for d in m.group(1).split(";"))):
            t = re.fullmatch(r"(%s)\s+(.+)" % "|".join(sorted(SCALARS, key=len, reverse=True)), decl, flags=re.S)
            for item in t.group(2).split(",") if t else [""]:
                f = re.fullmatch(r"\s*(\w+)\s*((?:\[\d+\])*)\s*", item)
                if not f:
                    raise HeaderError("include/orbfe.h: cannot read the field `%s` of %s" % (decl, m.group(2)))
                fields.append((f.group(1), t.group(1), tuple(int(d) for d in re.findall(r"\d+", f.group(2)))))
    text = re.sub(record, " ", text)
    handles = set(re.findall(r"typedef\s+struct\s+\w+\s+(\w+)\s*;", text))
    text = re.sub(r"typedef\s+struct\s+\w+\s+\w+\s*;", " ", text)
    pointees = handles | set(records) | {"void"}
    functions = {}
    for decl in filter(None, (d.strip() for d in text.split(";"))):
        m = re.fullmatch(r"(.*?)\b(orbfe_\w+)\s*\((.*)\)", decl, flags=re.S)
        if not m or m.group(2) in functions:
            raise HeaderError("include/orbfe.h: cannot read the declaration `%s`" % decl)
        params = [] if m.group(3).strip() == "void" else m.group(3).split(",")
        restype = None if m.group(1).strip() == "void" else _ctype(m.group(1), pointees, False)
        functions[m.group(2)] = (restype, [_ctype(p, pointees, True) for p in params])
    if len(functions) != ncalls:
        raise HeaderError("include/orbfe.h: %d functions read, but `orbfe_name(` occurs %d times" % (len(functions), ncalls))
    return functions, records, defines


with open(HEADER_PATH) as _f:
    functions, records, defines = _parse(_f.read())


def dtype(record):
    """The aligned np.dtype of a record of the header."""
    return np.dtype([(name, SCALARS[ctype], dims) if dims else (name, SCALARS[ctype]) for name, ctype, dims in records[record]],
                    align=True)


def structure(record):
    """The ctypes.Structure subclass of a record of the header (an array field: the nested ctypes array type)."""
    fields = []
    for name, ctype, dims in records[record]:
        t = SCALARS[ctype]
        for d in reversed(dims):
            t = t * d
        fields.append((name, t))
    return type(record, (C.Structure,), {"_fields_": fields, "__doc__": "%s (include/orbfe.h)." % record})
