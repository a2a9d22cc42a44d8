"""The list pass on a block (generate_mappings on carried lists, the edges call) adds nothing to the ABI: index 4 of
phmm_last_call_stats widens to the wide classes on mapping lists, documented in the header together with the developer
knob that holds the backward half to the generic kernel, and the symbol table is what it was.  No GPU needed."""
import os
import re

from dbgphmm_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "phmm_amd.h")) as f:
        return f.read()


def test_header_says_index_four_covers_the_list_pass():
    src = _header()
    doc = " ".join(src[src.index("---- instrumentation"):src.index("int phmm_last_call_stats")].replace("*", " ").split())
    assert re.search(r"4\s*=\s*the wide class of the hinted forward", doc)
    assert "Index 4 also covers the list pass" in doc
    assert "phmm_generate_mappings" in doc and "phmm_run_with_mapping_edges" in doc
    assert "PHMM_NO_WIDE_LIST_BWD" in doc and "PHMM_NO_WIDE_HINTED" in doc


def test_the_knob_is_read_with_the_others():
    with open(os.path.join(ROOT, "dbgphmm_amd", "csrc", "api.cpp")) as f:
        api = f.read()
    body = api[api.index("refresh_knobs"):]
    assert 'flag("PHMM_NO_WIDE_LIST_BWD")' in body[:body.index("\n}\n")]


def test_symbol_table_is_unchanged():
    src = _header()
    declared = sorted(set(re.findall(r"\b(phmm_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S))))
    assert declared == sorted(_ffi.DECLARED_SYMBOLS) and len(declared) == 55, len(declared)
    assert _ffi.PHMM_STATS_HINTED_WIDE == 4
