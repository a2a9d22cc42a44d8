"""The per-read backward total of generate_mappings (phmm_mappings_read_logp_backward) is part of the ABI: declared in
the header, exported by the library, bound in Python.  No GPU needed."""
import os
import re

import dbgphmm_amd as D
from dbgphmm_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_backward_total():
    with open(os.path.join(ROOT, "include", "phmm_amd.h")) as f:
        src = f.read()
    decl = re.search(r"int\s+phmm_mappings_read_logp_backward\s*\(([^)]*)\)\s*;", src)
    assert decl, "phmm_mappings_read_logp_backward is not declared"
    args = [a.strip() for a in decl.group(1).split(",")]
    assert args == ["const phmm_mappings *mp", "double *out_logp", "double *out_total"], args
    assert "phmm_mappings_read_logp_backward" in _ffi.DECLARED_SYMBOLS


def test_library_exports_backward_total():
    lib = _ffi.lib()
    assert hasattr(lib, "phmm_mappings_read_logp_backward")
    # NULL mappings: refused, nothing dereferenced
    assert lib.phmm_mappings_read_logp_backward(None, None, None) == _ffi.PHMM_EINVAL


def test_python_binding():
    assert callable(getattr(D.Mappings, "read_logp_backward", None))
    assert "backward" in D.Mappings.read_logp_backward.__doc__
