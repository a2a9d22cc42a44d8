"""ctypes prototypes of include/phmm_amd_edges.h (per-read transition usage over mapping lists: a sparse read-by-edge
matrix).

The tables of _ffi.py are closed; this companion header's symbols are listed and bound here, on the CDLL that
_ffi.lib() returns."""
from __future__ import annotations

import ctypes as C

from . import _ffi

# header -> symbols, as _ffi.EXTENSION_SYMBOLS
EDGES_SYMBOLS = {"phmm_amd_edges.h": ["phmm_run_with_mapping_read_edges", "phmm_read_edges_reads", "phmm_read_edges_keys",
                                      "phmm_read_edges_total", "phmm_read_edges_export", "phmm_read_edges_destroy"]}

PHMM_NO_KEY = 0xFFFFFFFF

_bound = None


def lib():
    """_ffi.lib() with the six entry points of phmm_amd_edges.h prototyped"""
    global _bound
    if _bound is not None:
        return _bound
    L = _ffi.lib()
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
    sig = {
        "phmm_run_with_mapping_read_edges": (i32, [vp, vp, vp, u32, vp, vp, vp, vp, vp, C.POINTER(vp)]),
        "phmm_read_edges_reads": (u64, [vp]),
        "phmm_read_edges_keys": (u64, [vp]),
        "phmm_read_edges_total": (u64, [vp]),
        "phmm_read_edges_export": (i32, [vp, vp, vp, vp]),
        "phmm_read_edges_destroy": (None, [vp]),
    }
    assert sorted(sig) == sorted(EDGES_SYMBOLS["phmm_amd_edges.h"])
    for name, (res, args) in sig.items():
        fn = getattr(L, name)  # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    _bound = L
    return L
