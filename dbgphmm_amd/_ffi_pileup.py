"""ctypes prototype of include/phmm_amd_pileup.h (pileup over mapping lists: per-node base evidence by state).

The tables of _ffi.py are closed; this companion header's symbol is listed and bound here, on the CDLL that
_ffi_usage.lib() returns: the rows come back as a phmm_read_usage handle, whose accessors _ffi_usage.py binds."""
from __future__ import annotations

import ctypes as C

from . import _ffi_usage

# header -> symbols, as _ffi.EXTENSION_SYMBOLS
PILEUP_SYMBOLS = {"phmm_amd_pileup.h": ["phmm_run_with_mapping_pileup"]}

_bound = None


def lib():
    """_ffi_usage.lib() with the entry point of phmm_amd_pileup.h prototyped"""
    global _bound
    if _bound is not None:
        return _bound
    L = _ffi_usage.lib()
    vp, i32 = C.c_void_p, C.c_int
    sig = {
        "phmm_run_with_mapping_pileup": (i32, [vp, vp, vp, vp, vp, C.POINTER(vp)]),
    }
    assert sorted(sig) == sorted(PILEUP_SYMBOLS["phmm_amd_pileup.h"])
    for name, (res, args) in sig.items():
        fn = getattr(L, name)  # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    _bound = L
    return L
