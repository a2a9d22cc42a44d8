"""The best path over mapping lists (phmm_run_with_mapping_best_path) is part of the ABI: declared in
include/phmm_amd_path.h (a companion header of phmm_amd.h, whose own symbol table is closed), exported by the library,
bound in Python, named in the documents.  No GPU needed."""
import os
import re

import dbgphmm_amd as D
from dbgphmm_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "phmm_amd_path.h"
SYMBOL = "phmm_run_with_mapping_best_path"


def _read(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def test_header_declares_best_path():
    src = _read("include", HEADER)
    decl = re.search(r"int\s+" + SYMBOL + r"\s*\(([^)]*)\)\s*;", src)
    assert decl, SYMBOL + " is not declared"
    args = [" ".join(a.split()) for a in decl.group(1).split(",")]
    assert args == ["phmm_model *m", "const phmm_reads *reads", "const phmm_mappings *mappings",
                    "double *out_logp", "uint32_t *out_path", "uint32_t *out_counts"], args
    assert '#include "phmm_amd.h"' in src
    assert re.search(r"#define\s+PHMM_PATH_NONE\s+0xffffffffu", src)
    assert re.search(r"#define\s+PHMM_PATH_INS_BEGIN\s+0xfffffffdu", src)
    assert D.PATH_NONE == 0xFFFFFFFF and D.PATH_INS_BEGIN == 0xFFFFFFFD
    # the header's symbols are exactly those the binding lists for it, and none of them is one of phmm_amd.h's
    declared = sorted(set(re.findall(r"\b(phmm_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S))))
    assert declared == sorted(_ffi.EXTENSION_SYMBOLS[HEADER]) == [SYMBOL]
    assert not set(declared) & set(_ffi.DECLARED_SYMBOLS)


def test_tie_rule_is_in_the_header():
    doc = _read("include", HEADER)
    at = doc.index("TIES.")
    assert at < doc.index("int " + SYMBOL) and "rank" in doc[at:at + 600]


def test_library_exports_best_path():
    lib = _ffi.lib()
    assert hasattr(lib, SYMBOL)
    # NULL model / reads / mappings: refused, nothing dereferenced
    assert getattr(lib, SYMBOL)(None, None, None, None, None, None) == _ffi.PHMM_EINVAL


def test_python_binding():
    fn = getattr(D.PHMMModel, "run_with_mapping_best_path", None)
    assert callable(fn) and callable(D.path_states)
    assert "best path" in fn.__doc__ and "counts" in fn.__doc__


def test_documents_name_it():
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert SYMBOL in _read(doc), doc
    assert "phmm_run_with_mapping_best_path" in _read("integration", "rust", "amd_sys.rs")
    assert "best_path_with_mapping_amd" in _read("integration", "rust", "amd.rs")
