"""The sampler's device-side state (phmm_likelihood: create / score_changes / move / current / refresh / destroy) is
part of the ABI: declared in the header with these argument lists, exported by the library, bound in Python.
No GPU needed."""
import ctypes as C
import os
import re

import numpy as np

import dbgphmm_amd as D
from dbgphmm_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLS = {
    "phmm_likelihood_create": ("int", ["phmm_model *m", "const phmm_reads *reads", "const phmm_mappings *mappings",
                                       "const uint32_t *copy_nums", "uint32_t min_copy_num", "phmm_likelihood **out"]),
    "phmm_likelihood_score_changes": ("int", ["phmm_likelihood *lk", "uint32_t n_candidates",
                                              "const uint64_t *change_off", "const uint32_t *change_node",
                                              "const uint32_t *change_copy_num", "double *out_logp",
                                              "double *out_total", "uint64_t *out_n_rescored"]),
    "phmm_likelihood_move": ("int", ["phmm_likelihood *lk", "uint64_t n_changes", "const uint32_t *change_node",
                                     "const uint32_t *change_copy_num", "double *out_total",
                                     "uint64_t *out_n_rescored"]),
    "phmm_likelihood_current": ("int", ["const phmm_likelihood *lk", "uint32_t *out_copy_nums", "double *out_logp",
                                        "double *out_total"]),
    "phmm_likelihood_refresh": ("int", ["phmm_likelihood *lk"]),
    "phmm_likelihood_destroy": ("void", ["phmm_likelihood *lk"]),
}


def test_header_declares_the_handle():
    with open(os.path.join(ROOT, "include", "phmm_amd.h")) as f:
        src = f.read()
    assert re.search(r"typedef\s+struct\s+phmm_likelihood\s+phmm_likelihood\s*;", src)
    for name, (ret, want) in DECLS.items():
        decl = re.search(ret + r"\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert decl, name + " is not declared"
        args = [" ".join(a.split()) for a in decl.group(1).split(",")]
        assert args == want, (name, args)
        assert name in _ffi.DECLARED_SYMBOLS
    assert "must outlive" in src  # the handle borrows model, reads and mappings


def test_library_exports_and_refuses_null():
    lib = _ffi.lib()
    for name in DECLS:
        assert hasattr(lib, name), name
    out = C.c_void_p(0x1234)
    cn = np.ones(4, np.uint32)
    sentinel = np.full(2, 7.0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    # NULL model / NULL out: refused, nothing dereferenced
    assert lib.phmm_likelihood_create(None, None, None, p(cn), 0, C.byref(out)) == _ffi.PHMM_EINVAL
    assert not out.value  # no handle behind a refusal
    assert lib.phmm_likelihood_create(None, None, None, None, 0, None) == _ffi.PHMM_EINVAL
    off = np.array([0, 1], np.uint64)
    assert lib.phmm_likelihood_score_changes(None, 1, p(off), p(cn), p(cn), None, p(sentinel),
                                             None) == _ffi.PHMM_EINVAL
    assert lib.phmm_likelihood_score_changes(None, 0, None, None, None, None, None, None) == _ffi.PHMM_EINVAL
    assert lib.phmm_likelihood_move(None, 1, p(cn), p(cn), p(sentinel), None) == _ffi.PHMM_EINVAL
    assert lib.phmm_likelihood_move(None, 0, None, None, None, None) == _ffi.PHMM_EINVAL
    assert lib.phmm_likelihood_current(None, p(cn), None, p(sentinel)) == _ffi.PHMM_EINVAL
    assert lib.phmm_likelihood_refresh(None) == _ffi.PHMM_EINVAL
    lib.phmm_likelihood_destroy(None)
    assert np.all(sentinel == 7.0) and np.all(cn == 1)
    assert b"NULL" in lib.phmm_last_error()


def test_python_binding():
    assert isinstance(D.Likelihood, type)
    assert "posterior.rs:314-417" in D.Likelihood.__doc__
    fn = getattr(D.PHMMModel, "likelihood", None)
    assert callable(fn) and "posterior.rs:247-255" in fn.__doc__
    assert "posterior.rs:470-528" in D.Likelihood.score_changes.__doc__
    assert "posterior.rs:532-600" in D.Likelihood.move.__doc__
    for name in ("score_changes", "move", "current", "refresh"):
        assert callable(getattr(D.Likelihood, name))
