"""Posterior path sampling over mapping lists (phmm_run_with_mapping_sample_paths) is part of the ABI: declared in
include/phmm_amd_sample.h (a companion header of phmm_amd.h, whose own symbol table is closed) with the random stream
and the draw rule written out, exported by the library, bound in Python, named in the documents.  No GPU needed."""
import os
import re

import dbgphmm_amd as D
from dbgphmm_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "phmm_amd_sample.h"
SYMBOL = "phmm_run_with_mapping_sample_paths"


def _read(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def test_header_declares_sample_paths():
    src = _read("include", HEADER)
    decl = re.search(r"int\s+" + SYMBOL + r"\s*\(([^)]*)\)\s*;", src)
    assert decl, SYMBOL + " is not declared"
    args = [" ".join(a.split()) for a in decl.group(1).split(",")]
    assert args == ["phmm_model *m", "const phmm_reads *reads", "const phmm_mappings *mappings", "uint32_t n_samples",
                    "uint64_t seed", "double *out_logp", "double *out_path_logp", "uint32_t *out_path",
                    "uint32_t *out_counts", "uint32_t *out_node_usage"], args
    assert '#include "phmm_amd.h"' in src
    assert re.search(r"#define\s+PHMM_SAMPLE_MAX\s+64\b", src)
    # the header's symbols are exactly those the binding lists for it, and none of them is one of phmm_amd.h's
    declared = sorted(set(re.findall(r"\b(phmm_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S))))
    assert declared == sorted(_ffi.EXTENSION_SYMBOLS[HEADER]) == [SYMBOL]
    assert not set(declared) & set(_ffi.DECLARED_SYMBOLS)


def test_stream_and_draw_rule_are_in_the_header():
    doc = _read("include", HEADER)
    decl = doc.index("int " + SYMBOL)
    at = doc.index("THE RANDOM STREAM.")
    assert at < decl
    stream = doc[at:doc.index("THE DRAW RULE.")]
    for word in ("SplitMix64", "0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB", "r * 64 + s + GOLD",
                 ">> 11", "2^-53", "not in a chunk"):
        assert word in stream, word
    at = doc.index("THE DRAW RULE.")
    rule = doc[at:decl]
    for word in ("running sum", "u * c_last < c_i", "last candidate with w > 0", "exactly one draw", "ascending edge index",
                 "InsBegin has one predecessor and consumes no draw"):
        assert word in rule, word
    assert "DUPLICATES." in doc[:decl] and "FIRST entry only" in doc[:decl]


def test_library_exports_sample_paths():
    lib = _ffi.lib()
    assert hasattr(lib, SYMBOL)
    # NULL model / reads / mappings: refused, nothing dereferenced
    assert getattr(lib, SYMBOL)(None, None, None, 4, 1, None, None, None, None, None) == _ffi.PHMM_EINVAL


def test_python_binding():
    fn = getattr(D.PHMMModel, "run_with_mapping_sample_paths", None)
    assert callable(fn)
    for word in ("posterior", "seed", "path_logp", "counts", "usage", "path_states"):
        assert word in fn.__doc__, word
    import inspect
    assert list(inspect.signature(fn).parameters) == ["self", "reads", "mappings", "n_samples", "seed", "want_path", "want_usage"]


def test_documents_name_it():
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert SYMBOL in _read(doc), doc
    assert "Path samples over the lists" in _read("DESIGN.md")
    assert SYMBOL in _read("integration", "rust", "amd_sys.rs")
    assert "sample_paths_with_mapping_amd" in _read("integration", "rust", "amd.rs")
    assert os.path.exists(os.path.join(ROOT, "tools", "sample_paths_time.py"))
    assert os.path.exists(os.path.join(ROOT, "profiles", "sample_paths.txt"))
