"""Per-read usage over mapping lists (phmm_run_with_mapping_read_usage and the phmm_read_usage handle) is part of the ABI:
declared in include/phmm_amd_usage.h (the ninth companion header of phmm_amd.h, whose own symbol table is closed) with
the keys, the rows and the order of the sums written out, exported by the library, bound in dbgphmm_amd/_ffi_usage.py
(the tables of _ffi.py stay as they are), named in the documents.  No GPU needed."""
import inspect
import os
import re

import dbgphmm_amd as D
from dbgphmm_amd import _ffi, _ffi_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "phmm_amd_usage.h"
SIGNATURES = {
    "phmm_run_with_mapping_read_usage": ("int", ["phmm_model *m", "const phmm_reads *reads", "const phmm_mappings *mappings",
                                                 "uint32_t n_groups", "const uint64_t *group_off",
                                                 "const uint32_t *group_nodes", "double *out_logp_forward",
                                                 "double *out_key_usage", "phmm_read_usage **out"]),
    "phmm_read_usage_reads": ("uint64_t", ["const phmm_read_usage *u"]),
    "phmm_read_usage_keys": ("uint64_t", ["const phmm_read_usage *u"]),
    "phmm_read_usage_total": ("uint64_t", ["const phmm_read_usage *u"]),
    "phmm_read_usage_export": ("int", ["const phmm_read_usage *u", "uint64_t *row_off", "uint32_t *keys", "double *usage"]),
    "phmm_read_usage_destroy": ("void", ["phmm_read_usage *u"]),
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
    assert '#include "phmm_amd.h"' in src and re.search(r"typedef\s+struct\s+phmm_read_usage\s+phmm_read_usage\s*;", code)
    declared = sorted(set(re.findall(r"\b(phmm_[a-z_0-9]+)\s*\(", code)))
    assert declared == sorted(SIGNATURES) == sorted(_ffi_usage.USAGE_SYMBOLS[HEADER])
    assert list(_ffi_usage.USAGE_SYMBOLS) == [HEADER]


def test_the_closed_tables_stay_closed():
    new = set(SIGNATURES)
    assert not new & set(_ffi.DECLARED_SYMBOLS)
    assert not new & {s for syms in _ffi.EXTENSION_SYMBOLS.values() for s in syms}
    assert HEADER not in _ffi.EXTENSION_SYMBOLS
    assert "read_usage" not in _read("include", "phmm_amd.h")


def test_contract_is_written_out_in_the_header():
    doc = _read("include", HEADER)
    decl = doc.index("int phmm_run_with_mapping_read_usage")
    text = " ".join(doc[:decl].replace("\n *", " ").split())
    for word in ("KEYS.", "n_groups == 0", "K = N", "phmm_likelihood_set_groups", "K = n_groups", "A node in no group has no key",
                 "Empty groups are allowed", "ROW of read r", "in ascending order", "counts twice", "exp(state_logp[a][s])",
                 "exp(-inf) is exactly 0", "stays, with zeros", "to_node_freqs()", "to_state_probs()", "out_key_usage[K][3]",
                 "a key in no row gets 0", "bit for bit", "ORDER OF THE SUMS.", "depends on its segment alone",
                 "no floating-point atomics", "n <= 64", "d = 32, 16, 8, 4, 2, 1", "repeated calls return the same bits",
                 "NULL, a host pointer or a device pointer", "out == NULL", "owns its device buffers and borrows nothing",
                 "*out left as it was", "PHMM_ECAPACITY", "24 bytes per list entry", "NO READS", "a handle of 0 rows",
                 "32 bytes per list entry of a chunk", "chunks of consecutive whole reads", "Index 2 of phmm_last_call_stats",
                 "has no knob of its own"):
        assert word in text, word


def test_library_exports_them():
    lib = _ffi_usage.lib()
    for name in SIGNATURES:
        assert hasattr(lib, name), name
    # NULL model / reads / mappings: refused, nothing dereferenced; NULL handles are empty
    assert lib.phmm_run_with_mapping_read_usage(None, None, None, 0, None, None, None, None, None) == _ffi.PHMM_EINVAL
    assert lib.phmm_run_with_mapping_read_usage(None, None, None, 3, None, None, None, None, None) == _ffi.PHMM_EINVAL
    assert lib.phmm_read_usage_reads(None) == 0 and lib.phmm_read_usage_keys(None) == 0
    assert lib.phmm_read_usage_total(None) == 0
    assert lib.phmm_read_usage_export(None, None, None, None) == _ffi.PHMM_EINVAL
    lib.phmm_read_usage_destroy(None)


def test_python_binding():
    fn = getattr(D.PHMMModel, "run_with_mapping_read_usage", None)
    assert callable(fn)
    sig = inspect.signature(fn).parameters
    assert list(sig) == ["self", "reads", "mappings", "groups", "want_totals"]
    assert sig["groups"].default is None and sig["want_totals"].default is True
    for word in ("include/phmm_amd_usage.h", "to_state_probs", "ReadUsage", "groups", "totals"):
        assert word in fn.__doc__, word
    for method in ("arrays", "row", "state_probs", "node_freqs", "reads_of", "from_arrays"):
        assert callable(getattr(D.ReadUsage, method, None)), method
    # from_arrays and the views, on the host alone
    import numpy as np
    u = D.ReadUsage.from_arrays(4, [0, 2, 2, 3], [1, 3, 1], [[.5, 0, .25], [1, 1, 1], [.25, .5, 0]], totals=np.zeros((4, 3)))
    assert len(u) == 3 and u.n_keys == 4 and u.totals.shape == (4, 3)
    assert u.row(0)[0].tolist() == [1, 3] and u.row(1)[0].size == 0
    assert u.state_probs(2).tolist() == [[0, 0, 0], [.25, .5, 0], [0, 0, 0], [0, 0, 0]]
    assert u.node_freqs(0).tolist() == [0, .75, 0, 3]
    reads, usage = u.reads_of(1)
    assert reads.tolist() == [0, 2] and usage.tolist() == [[.5, 0, .25], [.25, .5, 0]]
    assert u.reads_of(2)[0].size == 0


def test_documents_name_it():
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "phmm_run_with_mapping_read_usage" in _read(doc), doc
    assert "Read usage over the lists" in _read("DESIGN.md")
    rust = _read("integration", "rust", "amd_sys.rs")
    for name in SIGNATURES:
        assert name in rust, name
    assert os.path.exists(os.path.join(ROOT, "tools", "read_usage_time.py"))
    assert os.path.exists(os.path.join(ROOT, "profiles", "read_usage.txt"))
    assert "read_usage.hip" in _read("dbgphmm_amd", "csrc", "Makefile")
