"""The tables over mapping lists are part of the ABI: declared in include/phmm_amd_tables.h (the eighth companion header
of phmm_amd.h, whose own symbol table is closed) with the whole contract written out, exported by the library, bound in
dbgphmm_amd/_ffi_tables.py (the tables of _ffi.py stay closed), named in the documents.  No GPU needed."""
import os
import re

import dbgphmm_amd as D
from dbgphmm_amd import _ffi, _ffi_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "phmm_amd_tables.h"
SIGNATURES = {
    "phmm_run_with_mapping_tables": ["phmm_model *m", "const phmm_reads *reads", "const phmm_mappings *mappings",
                                     "double *out_logp_forward", "double *out_logp_backward", "double *out_forward",
                                     "double *out_forward_scalars", "double *out_backward", "double *out_backward_scalars"],
}


def _read(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def test_header_declares_the_entry_point():
    src = _read("include", HEADER)
    assert '#include "phmm_amd.h"' in src
    for name, want in SIGNATURES.items():
        decl = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert decl, name + " is not declared"
        assert [" ".join(a.split()) for a in decl.group(1).split(",")] == want, name
    declared = sorted(set(re.findall(r"\b(phmm_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S))))
    assert declared == sorted(SIGNATURES) == sorted(_ffi_tables.TABLES_SYMBOLS[HEADER])
    assert list(_ffi_tables.TABLES_SYMBOLS) == [HEADER]
    known = set(_ffi.DECLARED_SYMBOLS) | {s for syms in _ffi.EXTENSION_SYMBOLS.values() for s in syms}
    assert not set(declared) & known  # the closed tables stay closed


def test_the_contract_is_in_the_header():
    doc = _read("include", HEADER)
    for clause in ("THE MERGED INDEX", "it is NOT B.table_merged(p + 1)", "F.tables[p].mb is 0", "B.tables[p].e is 0",
                   "b_init", "PHMM_EINVAL", "PHMM_ECAPACITY", "more than 400 nodes", "node degree above 8",
                   "names a node twice", "a result, not a refusal", "No reads: nothing is written",
                   "same bits as the matching scalar", "is not run", "phmm_set_stream"):
        assert clause in doc, clause
    assert doc.index("THE MERGED INDEX") < doc.index("int phmm_run_with_mapping_tables")


def test_library_exports_it():
    lib = _ffi_tables.lib()
    # NULL model / reads / mappings: refused, nothing dereferenced
    assert lib.phmm_run_with_mapping_tables(None, None, None, None, None, None, None, None, None) == _ffi.PHMM_EINVAL


def test_python_binding():
    fn = getattr(D.PHMMModel, "run_with_mapping_tables", None)
    assert callable(fn) and "include/phmm_amd_tables.h" in fn.__doc__
    assert D.ListTables is not None and callable(D.ListTables.from_arrays)
    for name in ("forward", "backward", "table_merged", "prefix_logp", "suffix_logp", "ins_begin_posterior", "top_states"):
        assert callable(getattr(D.ListTables, name)), name


def test_documents_name_it():
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        for name in SIGNATURES:
            assert name in _read(doc), (doc, name)
    for name in SIGNATURES:
        assert name in _read("integration", "rust", "amd_sys.rs")
    assert "tables_with_mapping_amd" in _read("integration", "rust", "amd.rs")
