"""Per-read transition usage over mapping lists (phmm_run_with_mapping_read_edges and the phmm_read_edges handle) is part
of the ABI: declared in include/phmm_amd_edges.h (the tenth companion header of phmm_amd.h, whose own symbol table is
closed) with the keys, the rows, the end-term formula, the order of the sums and the refusals written out, exported by
the library, bound in dbgphmm_amd/_ffi_edges.py (the tables of _ffi.py stay as they are), named in the documents.
No GPU needed."""
import inspect
import os
import re

import dbgphmm_amd as D
from dbgphmm_amd import _ffi, _ffi_edges

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "phmm_amd_edges.h"
SIGNATURES = {
    "phmm_run_with_mapping_read_edges": ("int", ["phmm_model *m", "const phmm_reads *reads", "const phmm_mappings *mappings",
                                                 "uint32_t n_keys", "const uint32_t *edge_key", "const uint32_t *init_key",
                                                 "double *out_logp_forward", "double *out_end_terms",
                                                 "double *out_key_usage", "phmm_read_edges **out"]),
    "phmm_read_edges_reads": ("uint64_t", ["const phmm_read_edges *u"]),
    "phmm_read_edges_keys": ("uint64_t", ["const phmm_read_edges *u"]),
    "phmm_read_edges_total": ("uint64_t", ["const phmm_read_edges *u"]),
    "phmm_read_edges_export": ("int", ["const phmm_read_edges *u", "uint64_t *row_off", "uint32_t *keys", "double *usage"]),
    "phmm_read_edges_destroy": ("void", ["phmm_read_edges *u"]),
}


def _read(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def test_header_declares_the_six_symbols():
    """Fails without the feature: the header does not exist."""
    src = _read("include", HEADER)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, (res, want) in SIGNATURES.items():
        decl = re.search(r"\b" + res + r"\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert decl, name + " is not declared"
        assert [" ".join(a.split()) for a in decl.group(1).split(",")] == want, name
    assert '#include "phmm_amd.h"' in src and re.search(r"typedef\s+struct\s+phmm_read_edges\s+phmm_read_edges\s*;", code)
    assert re.search(r"#define\s+PHMM_NO_KEY\s+0xffffffffu", code) and _ffi_edges.PHMM_NO_KEY == 0xFFFFFFFF == D.PHMM_NO_KEY
    declared = sorted(set(re.findall(r"\b(phmm_[a-z_0-9]+)\s*\(", code)))
    assert declared == sorted(SIGNATURES) == sorted(_ffi_edges.EDGES_SYMBOLS[HEADER])
    assert list(_ffi_edges.EDGES_SYMBOLS) == [HEADER]


def test_the_closed_tables_stay_closed():
    new = set(SIGNATURES)
    assert not new & set(_ffi.DECLARED_SYMBOLS)
    assert not new & {s for syms in _ffi.EXTENSION_SYMBOLS.values() for s in syms}
    assert HEADER not in _ffi.EXTENSION_SYMBOLS
    assert "read_edges" not in _read("include", "phmm_amd.h")


def test_contract_is_written_out_in_the_header():
    doc = _read("include", HEADER)
    decl = doc.index("int phmm_run_with_mapping_read_edges")
    text = " ".join(doc[:decl].replace("\n *", " ").split())
    for word in (
            # the key rule
            "KEYS.", "n_keys == 0", "the key of edge e is e", "E + v", "K = E + N", "K = n_keys", "PHMM_NO_KEY",
            "Either array may be NULL", "may share a key", "their terms add",
            # the row rule
            "ROW of read r", "in ascending order", "the six transition kinds of to_edge_and_init_freqs",
            "phmm_run_dense_edges", "is NOT recorded by the pass and is not in the row",
            "phmm_run_with_mapping_read_usage", "A key absent from the row counts as 0",
            # the end-term formula
            "END TERMS.", "m = d = p_end on every node", "out_end_terms[r][0] = A_r", "out_end_terms[r][1] = T_r",
            "init_v * (A_r + T_r * e_v(x_last))", "A_r = p_ID * p_end * ib_{L-1} / P", "T_r = c_M * p_end * ib_{L-2} / P",
            "c_M = p_IM", "T_r = p_MM * p_end / P", "L == 1",
            # the other outputs
            "bit for bit", "out_key_usage[K]", "the end terms excluded", "a key in no row gets 0", "out_edge_freq",
            "out_init_freq[v]", "up to the order of the sums", "out == NULL",
            # the order of the sums
            "ORDER OF THE SUMS.", "depends on its segment alone", "no floating-point atomics", "in record order", "n <= 64",
            "d = 32, 16, 8, 4, 2, 1", "always by the second rule",
            # what is promised about bits
            "BITS.", "not on the other reads of the call", "repeated calls return the same bits", "agree to rounding only",
            "PHMM_WIDE_EDGE_BWD",
            # the refusals and the rest
            "NULL, a host pointer or a device pointer", "owns its device buffers and borrows nothing", "REFUSALS",
            "*out left as it was", "those of phmm_run_with_mapping_edges", "a read of probability 0 on its lists",
            "naming the read", "both NULL", "a value >= n_keys that is not PHMM_NO_KEY", "PHMM_ECAPACITY",
            "2^31 - 2 records or row entries", "NO READS", "a handle of 0 rows", "goes back when the call ends",
            "phmm_workspace_bytes() does not change", "32 bytes per record", "NOT chunked", "phmm_set_workspace_limit",
            "Index 2 of phmm_last_call_stats", "cells = records reduced", "has no knob of its own"):
        assert word in text, word


def test_library_exports_them():
    lib = _ffi_edges.lib()
    for name in SIGNATURES:
        assert hasattr(lib, name), name
    # NULL model / reads / mappings: refused, nothing dereferenced; NULL handles are empty
    assert lib.phmm_run_with_mapping_read_edges(None, None, None, 0, None, None, None, None, None, None) == _ffi.PHMM_EINVAL
    assert lib.phmm_run_with_mapping_read_edges(None, None, None, 3, None, None, None, None, None, None) == _ffi.PHMM_EINVAL
    assert lib.phmm_read_edges_reads(None) == 0 and lib.phmm_read_edges_keys(None) == 0
    assert lib.phmm_read_edges_total(None) == 0
    assert lib.phmm_read_edges_export(None, None, None, None) == _ffi.PHMM_EINVAL
    lib.phmm_read_edges_destroy(None)


def test_python_binding():
    fn = getattr(D.PHMMModel, "run_with_mapping_read_edges", None)
    assert callable(fn)
    sig = inspect.signature(fn).parameters
    assert list(sig)[:6] == ["self", "reads", "mappings", "edge_key", "init_key", "n_keys"]
    assert sig["edge_key"].default is None and sig["init_key"].default is None and sig["n_keys"].default == 0
    for word in ("include/phmm_amd_edges.h", "to_edge_and_init_freqs", "ReadEdges", "edge_key", "init_key", "link_keys"):
        assert word in fn.__doc__, word
    for method in ("arrays", "export", "row", "reads_of", "edge_freqs", "init_freqs", "from_arrays"):
        assert callable(getattr(D.ReadEdges, method, None)), method
    assert callable(D.link_keys)


def test_documents_name_it():
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "phmm_run_with_mapping_read_edges" in _read(doc), doc
    assert "Read edges over the lists" in _read("DESIGN.md")
    rust = _read("integration", "rust", "amd_sys.rs")
    for name in SIGNATURES:
        assert name in rust, name
    assert os.path.exists(os.path.join(ROOT, "tools", "read_edges_time.py"))
    assert os.path.exists(os.path.join(ROOT, "profiles", "read_edges.txt"))
    assert "read_edges.hip" in _read("dbgphmm_amd", "csrc", "Makefile")
