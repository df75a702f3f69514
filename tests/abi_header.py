"""The C declarations of include/srt_hip.h and include/srt_hip_test.h, parsed once for every test that compares the ctypes
prototypes of sexy-raytracer_amd/hipdev.py with them: the header reader, the parameter parser and the one table from C
spellings to ctypes types.

    struct pointer `T*` or `const T*`   POINTER(abi.T); c_void_p for a struct abi.py has no ctypes class of
    `void*`, `const void*`              c_void_p
    `char*`, `const char*`              c_char_p
    scalar pointer `float*`, ...        POINTER(c_float), ...
    `X name[4]`                         POINTER(X's type)
    scalars                             exact
    `SrtContext*`                       c_void_p (an opaque handle)"""
import ctypes as C
import os
import re

from conftest import ROOT

HEADERS = ("srt_hip.h", "srt_hip_test.h")
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint8_t": C.c_uint8, "uint64_t": C.c_uint64,
           "float": C.c_float}
RETURNS = dict(SCALARS, **{"void": None, "const char*": C.c_char_p})
_DECL = re.compile(r"\b((?:const\s+)?\w+\s*\*?)\s*(srt[A-Z]\w*)\s*\(([^)]*)\)\s*;")


def header(name=HEADERS[0]):
    return open(os.path.join(ROOT, "include", name)).read()


def declarations(name):
    """{function: (return type, [parameter types])} of one header, the types spelled `const T*`, `T* const[4]`, `int32_t`."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", header(name), flags=re.S)
    out = {}
    for ret, fn, args in _DECL.findall(text):
        params = []
        for arg in args.split(","):
            arg = " ".join(arg.split())
            arr = re.search(r"\[(\d+)\]$", arg)
            base = re.sub(r"\s*\w+(\[\d+\])?$", "", arg)  # drop the parameter name
            params.append(base.replace(" *", "*") + ("[%s]" % arr.group(1) if arr else ""))
        out[fn] = (" ".join(ret.split()).replace(" *", "*"), [] if params in ([""], ["void"]) else params)
    return out


def ctype(abi, spelling):
    """The table above: the ctypes type of one parameter as declarations() spells it."""
    arr = re.match(r"(.*?)(?: const)?\[\d+\]$", spelling)
    if arr:
        return C.POINTER(ctype(abi, arr.group(1)))
    t = re.sub(r"^const ", "", spelling)
    if t in SCALARS:
        return SCALARS[t]
    assert t.endswith("*"), spelling
    if t in ("void*", "SrtContext*"):
        return C.c_void_p
    if t == "char*":
        return C.c_char_p
    inner = t[:-1]
    if inner in SCALARS or inner.endswith("*"):
        return C.POINTER(ctype(abi, inner))
    struct = getattr(abi, inner, None)  # (SrtAovRecord is a NumPy dtype only: its pointer is an address)
    return C.POINTER(struct) if struct else C.c_void_p


def prototype(name):
    """(return type, [parameter types]) of one function, from whichever header declares it."""
    for h in HEADERS:
        decls = declarations(h)
        if name in decls:
            return decls[name]
    raise AssertionError("%s is declared in neither header" % name)


def assert_prototype(dev, abi, name, untyped=None):
    """Every parameter's ctypes type is the table's: the strict rule.  untyped: a predicate on the parameter's spelling that
    says where c_void_p is accepted as well (the older wrappers pass addresses as integers).  Returns the spellings."""
    params = prototype(name)[1]
    got = getattr(dev.lib, name).argtypes or []
    assert len(got) == len(params), (name, params)
    for g, p in zip(got, params):
        assert g.__name__ == ctype(abi, p).__name__ or (untyped and untyped(p) and g is C.c_void_p), (name, p, g)
    return params
