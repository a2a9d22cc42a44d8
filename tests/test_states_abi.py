"""State posteriors over mapping lists (phmm_run_with_mapping_states) are part of the ABI: declared in
include/phmm_amd_states.h (the companion header of phmm_amd.h, whose own symbol table is closed), exported by the
library, bound in Python.  No GPU needed."""
import os
import re

import dbgphmm_amd as D
from dbgphmm_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "phmm_amd_states.h"


def _header():
    with open(os.path.join(ROOT, "include", HEADER)) as f:
        return f.read()


def test_header_declares_list_states():
    src = _header()
    decl = re.search(r"int\s+phmm_run_with_mapping_states\s*\(([^)]*)\)\s*;", src)
    assert decl, "phmm_run_with_mapping_states is not declared"
    args = [" ".join(a.split()) for a in decl.group(1).split(",")]
    assert args == ["phmm_model *m", "const phmm_reads *reads", "const phmm_mappings *mappings",
                    "double *out_logp_forward", "double *out_state_logp", "uint32_t *out_best"], args
    assert '#include "phmm_amd.h"' in src
    # the header's symbols are exactly those the binding lists for it, and none of them is one of phmm_amd.h's
    declared = sorted(set(re.findall(r"\b(phmm_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S))))
    assert declared == sorted(_ffi.EXTENSION_SYMBOLS[HEADER]) == ["phmm_run_with_mapping_states"]
    assert not set(declared) & set(_ffi.DECLARED_SYMBOLS)


def test_library_exports_list_states():
    lib = _ffi.lib()
    assert hasattr(lib, "phmm_run_with_mapping_states")
    # NULL model / reads / mappings: refused, nothing dereferenced
    assert lib.phmm_run_with_mapping_states(None, None, None, None, None, None) == _ffi.PHMM_EINVAL


def test_python_binding():
    fn = getattr(D.PHMMModel, "run_with_mapping_states", None)
    assert callable(fn)
    assert "to_emit_probs" in fn.__doc__ and "to_states" in fn.__doc__


def test_block_knob_is_documented():
    """the opt-in of the block backward is named in the comment on the declaration"""
    doc = _header()
    at = doc.index("PHMM_WIDE_STATES_BWD")
    assert at < doc.index("int phmm_run_with_mapping_states") < at + 1000
