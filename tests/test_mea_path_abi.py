"""The weighted walk and the MEA path over mapping lists are part of the ABI: declared in include/phmm_amd_mea.h (the
seventh companion header of phmm_amd.h, whose own symbol table is closed) with the whole contract written out, exported
by the library, bound in dbgphmm_amd/_ffi_mea.py (the tables of _ffi.py stay closed), named in the documents.  No GPU
needed."""
import os
import re

import dbgphmm_amd as D
from dbgphmm_amd import _ffi, _ffi_mea

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "phmm_amd_mea.h"
SIGNATURES = {
    "phmm_run_with_mapping_weighted_path": ["phmm_model *m", "const phmm_reads *reads", "const phmm_mappings *mappings",
                                            "const double *weights", "const double *ib_weight", "double *out_score",
                                            "uint32_t *out_path", "uint32_t *out_counts"],
    "phmm_run_with_mapping_mea_path": ["phmm_model *m", "const phmm_reads *reads", "const phmm_mappings *mappings",
                                       "double del_weight", "double *out_logp_forward", "double *out_score",
                                       "uint32_t *out_path", "uint32_t *out_counts", "double *out_weights"],
}


def _read(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def test_header_declares_both_entry_points():
    src = _read("include", HEADER)
    assert '#include "phmm_amd.h"' in src
    for name, want in SIGNATURES.items():
        decl = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert decl, name + " is not declared"
        assert [" ".join(a.split()) for a in decl.group(1).split(",")] == want, name
    declared = sorted(set(re.findall(r"\b(phmm_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S))))
    assert declared == sorted(SIGNATURES) == sorted(_ffi_mea.MEA_SYMBOLS[HEADER])
    assert list(_ffi_mea.MEA_SYMBOLS) == [HEADER]
    known = set(_ffi.DECLARED_SYMBOLS) | {s for syms in _ffi.EXTENSION_SYMBOLS.values() for s in syms}
    assert not set(declared) & known  # the closed tables stay closed


def test_the_contract_is_in_the_header():
    doc = _read("include", HEADER)
    for clause in ("ADMISSIBLE.", "VALUES.", "TIES", "fl(source value + own weight)", "InsBegin has weight 0",
                   "PHMM_ECAPACITY", "NaN or infinite", "del_weight must be finite and >= 0"):
        assert clause in doc, clause
    assert doc.index("TIES") < doc.index("int phmm_run_with_mapping_weighted_path")


def test_library_exports_them():
    lib = _ffi_mea.lib()
    # NULL model / reads / mappings: refused, nothing dereferenced
    assert lib.phmm_run_with_mapping_weighted_path(None, None, None, None, None, None, None, None) == _ffi.PHMM_EINVAL
    assert lib.phmm_run_with_mapping_mea_path(None, None, None, 1.0, None, None, None, None, None) == _ffi.PHMM_EINVAL


def test_python_binding():
    for name in ("run_with_mapping_weighted_path", "run_with_mapping_mea_path"):
        fn = getattr(D.PHMMModel, name, None)
        assert callable(fn) and "include/phmm_amd_mea.h" in fn.__doc__, name


def test_documents_name_them():
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        for name in SIGNATURES:
            assert name in _read(doc), (doc, name)
    for name in SIGNATURES:
        assert name in _read("integration", "rust", "amd_sys.rs")
    assert "mea_path_with_mapping_amd" in _read("integration", "rust", "amd.rs")
