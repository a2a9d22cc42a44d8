"""Reads drawn from the model (phmm_sample_reads) are part of the ABI: declared in include/phmm_amd_generate.h (a
companion header of phmm_amd.h, whose own symbol table is closed) with the walk, the random stream and the draw rule
written out, exported by the library, bound in Python, named in the documents.  No GPU needed."""
import inspect
import os
import re

import dbgphmm_amd as D
from dbgphmm_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "phmm_amd_generate.h"
SYMBOL = "phmm_sample_reads"


def _read(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def test_header_declares_sample_reads():
    src = _read("include", HEADER)
    decl = re.search(r"int\s+" + SYMBOL + r"\s*\(([^)]*)\)\s*;", src)
    assert decl, SYMBOL + " is not declared"
    args = [" ".join(a.split()) for a in decl.group(1).split(",")]
    assert args == ["phmm_model *m", "uint64_t first_index", "uint64_t n_walks", "uint32_t length", "uint32_t length_kind",
                    "const uint32_t *start_nodes", "uint64_t n_start_nodes", "uint64_t seed", "uint8_t *out_bases",
                    "uint32_t *out_len", "uint32_t *out_flags", "uint32_t *out_history", "uint32_t history_cap",
                    "uint32_t *out_history_len", "uint32_t *out_node_usage"], args
    assert '#include "phmm_amd.h"' in src
    for name, value in (("PHMM_GEN_STATE_COUNT", "0u"), ("PHMM_GEN_ENDABLE", "1u"), ("PHMM_GEN_EMIT_COUNT", "2u"),
                        ("PHMM_GEN_END", "0xfffffffcu"), ("PHMM_GEN_ENDED", "1u"), ("PHMM_GEN_DEAD_END", "2u"),
                        ("PHMM_GEN_STATE_CAP", "4u"), ("PHMM_GEN_HISTORY_TRUNCATED", "8u")):
        assert re.search(r"#define\s+" + name + r"\s+" + value + r"\b", src), name
    # the header's symbols are exactly those the binding lists for it, and none of them is one of phmm_amd.h's
    declared = sorted(set(re.findall(r"\b(phmm_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S))))
    assert declared == sorted(_ffi.EXTENSION_SYMBOLS[HEADER]) == [SYMBOL]
    assert not set(declared) & set(_ffi.DECLARED_SYMBOLS)
    # the other four companion headers keep their entries
    assert _ffi.EXTENSION_SYMBOLS["phmm_amd_states.h"] == ["phmm_run_with_mapping_states"]
    assert _ffi.EXTENSION_SYMBOLS["phmm_amd_path.h"] == ["phmm_run_with_mapping_best_path"]
    assert _ffi.EXTENSION_SYMBOLS["phmm_amd_share.h"] == ["phmm_last_call_prefix_share"]
    assert _ffi.EXTENSION_SYMBOLS["phmm_amd_sample.h"] == ["phmm_run_with_mapping_sample_paths"]
    assert len(_ffi.EXTENSION_SYMBOLS) == 5


def test_stream_and_draw_rule_are_in_the_header():
    doc = _read("include", HEADER)
    decl = doc.index("int " + SYMBOL)
    at = doc.index("THE RANDOM STREAM.")
    assert doc.index("THE WALK.") < at < decl
    stream = doc[at:doc.index("THE DRAW RULE.")]
    for word in ("SplitMix64", "0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB",
                 "x0 = mix(seed ^ mix(i + GOLD))", ">> 11", "2^-53", "first_index + w"):
        assert word in stream, word
    rule = doc[doc.index("THE DRAW RULE."):decl]
    for word in ("running sum", "u * c_last < c_i", "last candidate with w > 0", "exactly one draw"):
        assert word in rule, word
    walk = doc[doc.index("THE WALK."):at]
    for word in ("ascending edge index", "Match(child), Ins(v), Del(child)", "InsBegin, Match(v), Del(v)", "p_II, p_IM, p_ID",
                 "8 * length + 64", "no draw is consumed", "even when Ins is chosen"):
        assert word in walk, word


def test_library_exports_sample_reads():
    lib = _ffi.lib()
    assert hasattr(lib, SYMBOL)
    # NULL model: refused, nothing dereferenced
    assert getattr(lib, SYMBOL)(None, 0, 4, 10, 0, None, 0, 1, None, None, None, None, 0, None, None) == _ffi.PHMM_EINVAL


def test_python_binding():
    fn = getattr(D.PHMMModel, "sample_reads", None)
    assert callable(fn)
    assert list(inspect.signature(fn).parameters) == ["self", "length", "kind", "n_reads", "total_bases", "start_nodes", "seed",
                                                      "want_history", "batch"]
    sig = inspect.signature(fn).parameters
    assert sig["kind"].default == "state_count" and sig["batch"].default == 4096 and sig["seed"].default == 0
    for word in ("sample_by_profile", "emit_count", "walk_index", "flags", "history", "batch"):
        assert word in fn.__doc__, word


def test_documents_name_it():
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert SYMBOL in _read(doc), doc
    design = _read("DESIGN.md")
    assert "Reads drawn from the model" in design
    assert "sample.rs:168-419" in design and "picker.rs:10-44" in design
    assert SYMBOL in _read("integration", "rust", "amd_sys.rs")
    assert "sample_reads_amd" in _read("integration", "rust", "amd.rs")
    assert SYMBOL in _read("tools", "sample_reads_time.py") or "sample_reads_raw" in _read("tools", "sample_reads_time.py")
    assert "sample_reads" in _read("profiles", "sample_reads.txt")
