"""ctypes prototypes of include/phmm_amd_align.h (alignment records: CIGAR and node walk of best and sampled paths).

The tables of _ffi.py are closed; this companion header's symbols are listed and bound here, on the CDLL that
_ffi.lib() returns."""
from __future__ import annotations

import ctypes as C

from . import _ffi

PHMM_ALN_INS, PHMM_ALN_DEL, PHMM_ALN_EQ, PHMM_ALN_DIFF = 1, 2, 7, 8  # the op values (BAM's)
OP_CHARS = {PHMM_ALN_INS: "I", PHMM_ALN_DEL: "D", PHMM_ALN_EQ: "=", PHMM_ALN_DIFF: "X"}

# header -> symbols, as _ffi.EXTENSION_SYMBOLS
ALIGN_SYMBOLS = {"phmm_amd_align.h": ["phmm_run_with_mapping_alignments", "phmm_alignments_count",
                                      "phmm_alignments_total_ops", "phmm_alignments_total_runs",
                                      "phmm_alignments_export", "phmm_alignments_destroy"]}

_bound = None


def lib():
    """_ffi.lib() with the six entry points of phmm_amd_align.h prototyped"""
    global _bound
    if _bound is not None:
        return _bound
    L = _ffi.lib()
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
    sig = {
        "phmm_run_with_mapping_alignments": (i32, [vp, vp, vp, u32, u64, vp, vp, vp, C.POINTER(vp)]),
        "phmm_alignments_count": (u64, [vp]),
        "phmm_alignments_total_ops": (u64, [vp]),
        "phmm_alignments_total_runs": (u64, [vp]),
        "phmm_alignments_export": (i32, [vp, vp, vp, vp, vp, vp]),
        "phmm_alignments_destroy": (None, [vp]),
    }
    assert sorted(sig) == sorted(ALIGN_SYMBOLS["phmm_amd_align.h"])
    for name, (res, args) in sig.items():
        fn = getattr(L, name)  # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    _bound = L
    return L
