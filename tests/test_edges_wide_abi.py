"""The edge-term backward on a block and the 128-thread size of the list backward add two environment knobs and nothing
to the ABI: both are read with the other knobs, and the header's instrumentation paragraph says what index 4 of
phmm_last_call_stats counts under them.  No GPU needed."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_knobs_are_read_with_the_others():
    with open(os.path.join(ROOT, "dbgphmm_amd", "csrc", "api.cpp")) as f:
        api = f.read()
    body = api[api.index("refresh_knobs"):]
    body = body[:body.index("\n}\n")]
    assert 'flag("PHMM_WIDE_EDGE_BWD")' in body
    assert 'num("PHMM_WIDE_BWD_T", 0)' in body
    # the edge-term backward is a knob of its own, not a part of PHMM_WIDE_HINTED
    line = next(l for l in body.splitlines() if "k.wide_hinted =" in l)
    assert "PHMM_WIDE_EDGE_BWD" not in line


def test_header_says_what_index_four_counts_under_the_knobs():
    with open(os.path.join(ROOT, "include", "phmm_amd.h")) as f:
        src = f.read()
    doc = " ".join(src[src.index("---- instrumentation"):src.index("int phmm_last_call_stats")].replace("*", " ").split())
    assert "PHMM_WIDE_EDGE_BWD=1" in doc and "PHMM_WIDE_BWD_T=128" in doc
    at = doc.index("PHMM_WIDE_EDGE_BWD")
    assert "phmm_run_with_mapping_edges" in doc[at:] and "backward" in doc[at:]
