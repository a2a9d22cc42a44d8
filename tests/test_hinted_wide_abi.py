"""The wide class of the hinted forward is visible at the ABI: phmm_last_call_stats takes which = 4 (documented in the
header, named in the Python binding) and nothing else about the symbol table changes.  No GPU needed."""
import ctypes as C
import os
import re

from dbgphmm_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stats(which):
    ms, n, c = C.c_double(-1.0), C.c_uint64(7), C.c_uint64(7)
    return _ffi.lib().phmm_last_call_stats(which, C.byref(ms), C.byref(n), C.byref(c)), ms.value, n.value, c.value


def test_stats_index_four_is_the_wide_hinted_class():
    # (what the figures are depends on the calls this process made before: only that they are written is checked)
    for which in range(5):
        rc, ms, n, c = _stats(which)
        assert rc == _ffi.PHMM_OK and ms >= 0.0, which
    assert _ffi.PHMM_STATS_HINTED_WIDE == 4
    ms, n, c = _ffi.last_call_stats(_ffi.PHMM_STATS_HINTED_WIDE)
    assert ms >= 0.0 and n >= 0 and c >= 0
    # NULL outputs are fine
    assert _ffi.lib().phmm_last_call_stats(4, None, None, None) == _ffi.PHMM_OK


def test_other_indices_are_refused():
    for which in (5, 6, 100, -1):
        rc, ms, n, c = _stats(which)
        assert rc == _ffi.PHMM_EINVAL and (ms, n, c) == (-1.0, 7, 7), which  # nothing written


def test_header_documents_the_class_and_the_symbol_table_is_unchanged():
    with open(os.path.join(ROOT, "include", "phmm_amd.h")) as f:
        src = f.read()
    doc = src[src.index("---- instrumentation"):src.index("int phmm_last_call_stats")]
    assert re.search(r"4\s*=\s*the wide class of the hinted forward", doc) and "PHMM_NO_WIDE_HINTED" in doc
    decl = re.search(r"int\s+phmm_last_call_stats\s*\(([^)]*)\)\s*;", src)
    assert [" ".join(a.split()) for a in decl.group(1).split(",")] == [
        "int which", "double *out_ms", "uint64_t *out_launches", "uint64_t *out_cells"]
    declared = sorted(set(re.findall(r"\b(phmm_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S))))
    assert declared == sorted(_ffi.DECLARED_SYMBOLS) and len(declared) == 55, len(declared)
