"""ctypes prototypes of include/phmm_amd_mea.h (the weighted walk over mapping lists and the maximum-expected-accuracy
path built on it).

The tables of _ffi.py are closed; this companion header's symbols are listed and bound here, on the CDLL that
_ffi.lib() returns."""
from __future__ import annotations

import ctypes as C

from . import _ffi

# header -> symbols, as _ffi.EXTENSION_SYMBOLS
MEA_SYMBOLS = {"phmm_amd_mea.h": ["phmm_run_with_mapping_weighted_path", "phmm_run_with_mapping_mea_path"]}

_bound = None


def lib():
    """_ffi.lib() with the two entry points of phmm_amd_mea.h prototyped"""
    global _bound
    if _bound is not None:
        return _bound
    L = _ffi.lib()
    vp, i32, dbl = C.c_void_p, C.c_int, C.c_double
    sig = {
        "phmm_run_with_mapping_weighted_path": (i32, [vp, vp, vp, vp, vp, vp, vp, vp]),
        "phmm_run_with_mapping_mea_path": (i32, [vp, vp, vp, dbl, vp, vp, vp, vp, vp]),
    }
    assert sorted(sig) == sorted(MEA_SYMBOLS["phmm_amd_mea.h"])
    for name, (res, args) in sig.items():
        fn = getattr(L, name)  # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    _bound = L
    return L
