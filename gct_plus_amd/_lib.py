"""ctypes binding of libgctplus_hip.so (C ABI: include/gctplus_hip.h).

The library is mandatory: there is no CPU / eager-PyTorch fallback.  `load()` raises
if the shared object is missing or does not export every declared symbol.
"""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GCT_LIB_PATH") or os.path.join(_HERE, "libgctplus_hip.so")   # override: A/B builds

INCLUDE_DIR = os.path.join(os.path.dirname(_HERE), "include")


class GctError(RuntimeError):
    pass


# The headers are the one definition of the boundary: every binding below is parsed from them at import.
# char* is a C string (bytes in, a string buffer, or a message out); every other pointer, a pointer to pointers or to
# a struct included, is an address.  A value type that is not listed is an error: nothing is bound by default.
_VALUE_TYPES = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float,
                "uint64_t": C.c_uint64, "uint32_t": C.c_uint32}
_PROTOTYPE = re.compile(r"([A-Za-z_][\w\s\*]*?)\b(\w+)\s*\(([^()]*)\)\s*;")


def _ctype(decl: str, proto: str, is_return: bool = False):
    words = decl.replace("*", " * ").split()
    if not is_return and len(words) > 1 and words[-1] != "*":
        words.pop()                                     # the parameter's name
    base = " ".join(w for w in words if w not in ("const", "*"))
    stars = words.count("*")
    if stars == 1 and base == "char":
        return C.c_char_p
    if stars and re.fullmatch(r"\w+", base):
        return C.c_void_p
    if not stars and base in _VALUE_TYPES:
        return _VALUE_TYPES[base]
    raise GctError(f"no ctypes binding for `{decl.strip()}` in `{proto}`")


def parse_prototypes(text: str) -> dict:
    """name -> (restype, [argtypes]) of every `ret name(args);` of a C header's text."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^\s*#.*$|extern\s+\"C\"\s*\{|typedef\s+struct\s*\w*\s*\{[^{}]*\}\s*\w+\s*;", " ", text, flags=re.M)
    out = {}
    for m in _PROTOTYPE.finditer(text):
        proto = " ".join(m.group(0).split())
        args = [] if m.group(3).strip() in ("", "void") else m.group(3).split(",")
        out[m.group(2)] = (_ctype(m.group(1), proto, is_return=True), [_ctype(a, proto) for a in args])
    rest = _PROTOTYPE.sub(" ", text).replace("}", " ").split()
    if rest:
        raise GctError(f"not a prototype: `{' '.join(rest)[:120]}`")
    return out


def _read_header(name: str) -> str:
    path = os.path.join(INCLUDE_DIR, name)
    try:
        with open(path, encoding="utf-8") as f:
            return f.read()
    except OSError as e:
        raise GctError(f"{path} is missing: it defines the bindings of {LIB_PATH}") from e


def _parse_header(name: str) -> dict:
    sigs = parse_prototypes(_read_header(name))
    if not sigs:
        raise GctError(f"no prototype found in {os.path.join(INCLUDE_DIR, name)}")
    return sigs


def _abi_version() -> int:
    m = re.search(r"^\s*#\s*define\s+GCT_ABI_VERSION\s+(\d+)\b", _read_header("gctplus_hip.h"), flags=re.M)
    if not m:
        raise GctError("include/gctplus_hip.h does not define GCT_ABI_VERSION")
    return int(m.group(1))


SIGNATURES = _parse_header("gctplus_hip.h")         # name -> (restype, [argtypes])
ABI_VERSION = _abi_version()
_lib = None


def load():
    """Load (once) and return the ctypes handle; hard error if unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GctError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` (or `make -C gct_plus_amd/csrc`). gct_plus_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise GctError(f"{LIB_PATH} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    if lib.gct_version() != ABI_VERSION:
        raise GctError(f"ABI mismatch: library {lib.gct_version()} != binding {ABI_VERSION}")
    _lib = lib
    return lib


# ---- the diagnostics library (include/gctplus_diag.h): separate from the operator boundary, optional at run time
DIAG_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libgctplus_diag.so")
DIAG_SIGNATURES = _parse_header("gctplus_diag.h")
_diag = None


def load_diag():
    """ctypes handle of libgctplus_diag.so (GctError if it is not built: callers treat that as "no diagnosis")."""
    global _diag
    if _diag is not None:
        return _diag
    if not os.path.exists(DIAG_PATH):
        raise GctError(f"{DIAG_PATH} is missing (make -C gct_plus_amd/csrc)")
    lib = C.CDLL(DIAG_PATH)
    for name, (res, args) in DIAG_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _diag = lib
    return lib


def check_diag(rc: int, what: str):
    if rc != 0:
        raise GctError(f"{what} failed (rc={rc}): {load_diag().gct_diag_last_error().decode('utf-8', 'replace')}")


_TRACE = os.environ.get("GCT_TRACE_OPS", "0") != "0"    # debugging aid: name every launch on stderr and drain the device
                                                        # after it, so that a faulting kernel is the last name printed


def check(rc: int, what: str):
    if rc != 0:
        msg = load().gct_last_error().decode("utf-8", "replace")
        raise GctError(f"{what} failed (rc={rc}): {msg}")
    if _TRACE:
        import sys
        import torch
        print(f"[gct] {what}", file=sys.stderr, flush=True)
        torch.cuda.synchronize()
