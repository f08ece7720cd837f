"""_lib.py against include/dtfill.h: every prototype's argument and return types, and every mirrored integer constant.
ctypes takes whatever argtypes it is given, so a c_float where the header says int would load and run; this is what stops it."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_TYPES = {"int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t, "unsigned": ctypes.c_uint,
           "long long": ctypes.c_longlong}


def _header():
    src = open(os.path.join(ROOT, "include", "dtfill.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return re.sub(r"//[^\n]*", "", src)


def _ctype(decl, returned=False):
    """`const float *x` -> c_void_p, `long long n` -> c_longlong, a returned `const char *` -> c_char_p."""
    if "*" in decl:
        if returned:
            assert decl.replace(" ", "") == "constchar*", decl
            return ctypes.c_char_p
        return ctypes.c_void_p
    words = decl.split()
    return C_TYPES[" ".join(words if returned else words[:-1])]  # (a parameter's last word is its name)


def _prototypes():
    """symbol -> (restype, argtypes) as the header declares them, in its order."""
    protos = {}
    for ret, name, params in re.findall(r"^([A-Za-z_][\w \t]*?[ \t*]+)(dtfill_\w+)\s*\(([^)]*)\)\s*;", _header(), flags=re.M):
        params = " ".join(params.split())
        args = [] if params == "void" else [_ctype(p.strip()) for p in params.split(",")]
        assert name not in protos, name
        protos[name] = (_ctype(ret.strip(), returned=True), args)
    return protos


def test_table_and_library_match_the_header(pkg):
    protos = _prototypes()
    assert list(protos) == list(pkg._lib._ABI) == list(pkg._lib.SYMBOLS)  # the header's order too
    pkg.build()
    L = pkg.load()
    for name, (restype, argtypes) in protos.items():
        assert pkg._lib._ABI[name] == (restype, argtypes), name
        f = getattr(L, name)
        assert (f.restype, list(f.argtypes)) == (restype, argtypes), name


def test_constants_match_the_header(pkg):
    lib = pkg._lib
    defines = {k: int(v.rstrip("u")) for k, v in re.findall(r"^#define DTFILL_(\w+)[ \t]+(-?\d+u?)\b", _header(), flags=re.M)}
    mirrored = [n for n in vars(lib) if re.match(r"(METRIC|FRAME|FLAG|LINES|READ|RGB|METRICS|LOSS)_[A-Z0-9_]+$", n)
                and isinstance(getattr(lib, n), int)]
    assert len(mirrored) == 21, sorted(mirrored)
    for n in mirrored:
        assert getattr(lib, n) == defines[n], n
    assert len(lib.STATS) == defines["STATS_N"]
    assert len(lib.METRICS_COLUMNS) == defines["METRICS_N"]
    assert len(lib.LOSS_COLUMNS) == defines["LOSS_N"]
