"""Transition posteriors over mapping lists (phmm_run_with_mapping_edges) are part of the ABI: declared in the header,
exported by the library, bound in Python.  No GPU needed."""
import os
import re

import dbgphmm_amd as D
from dbgphmm_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_list_edges():
    with open(os.path.join(ROOT, "include", "phmm_amd.h")) as f:
        src = f.read()
    decl = re.search(r"int\s+phmm_run_with_mapping_edges\s*\(([^)]*)\)\s*;", src)
    assert decl, "phmm_run_with_mapping_edges is not declared"
    args = [" ".join(a.split()) for a in decl.group(1).split(",")]
    assert args == ["phmm_model *m", "const phmm_reads *reads", "const phmm_mappings *mappings",
                    "double *out_logp_forward", "double *out_edge_freq", "double *out_init_freq"], args
    assert "phmm_run_with_mapping_edges" in _ffi.DECLARED_SYMBOLS


def test_library_exports_list_edges():
    lib = _ffi.lib()
    assert hasattr(lib, "phmm_run_with_mapping_edges")
    # NULL model / reads / mappings: refused, nothing dereferenced
    assert lib.phmm_run_with_mapping_edges(None, None, None, None, None, None) == _ffi.PHMM_EINVAL


def test_python_binding():
    fn = getattr(D.PHMMModel, "run_with_mapping_edge_freqs", None)
    assert callable(fn)
    assert "to_edge_and_init_freqs" in fn.__doc__
