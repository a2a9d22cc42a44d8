"""ctypes prototype of include/phmm_amd_tables.h (the forward and backward tables of the list pass, per list entry and
per base).

The tables of _ffi.py are closed; this companion header's symbol is listed and bound here, on the CDLL that
_ffi.lib() returns."""
from __future__ import annotations

import ctypes as C

from . import _ffi

# header -> symbols, as _ffi.EXTENSION_SYMBOLS
TABLES_SYMBOLS = {"phmm_amd_tables.h": ["phmm_run_with_mapping_tables"]}

_bound = None


def lib():
    """_ffi.lib() with the entry point of phmm_amd_tables.h prototyped"""
    global _bound
    if _bound is not None:
        return _bound
    L = _ffi.lib()
    vp, i32 = C.c_void_p, C.c_int
    sig = {
        "phmm_run_with_mapping_tables": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    }
    assert sorted(sig) == sorted(TABLES_SYMBOLS["phmm_amd_tables.h"])
    for name, (res, args) in sig.items():
        fn = getattr(L, name)  # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    _bound = L
    return L
