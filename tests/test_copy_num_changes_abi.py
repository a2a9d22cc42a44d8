"""Candidates as changes to a base copy-number vector (phmm_full_prob_reads_copy_num_changes) are part of the ABI:
declared in the header, exported by the library, bound in Python, with the CSR helper that builds the changes.
No GPU needed."""
import os
import re

import numpy as np

import dbgphmm_amd as D
from dbgphmm_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_copy_num_changes():
    with open(os.path.join(ROOT, "include", "phmm_amd.h")) as f:
        src = f.read()
    decl = re.search(r"int\s+phmm_full_prob_reads_copy_num_changes\s*\(([^)]*)\)\s*;", src)
    assert decl, "phmm_full_prob_reads_copy_num_changes is not declared"
    args = [" ".join(a.split()) for a in decl.group(1).split(",")]
    assert args == ["phmm_model *m", "const phmm_reads *reads", "const phmm_mappings *mappings",
                    "const uint32_t *base_copy_nums", "uint32_t min_copy_num", "uint32_t n_candidates",
                    "const uint64_t *change_off", "const uint32_t *change_node", "const uint32_t *change_copy_num",
                    "double *out_logp", "double *out_total", "uint64_t *out_n_rescored"], args
    assert "phmm_full_prob_reads_copy_num_changes" in _ffi.DECLARED_SYMBOLS


def test_library_exports_copy_num_changes():
    lib = _ffi.lib()
    assert hasattr(lib, "phmm_full_prob_reads_copy_num_changes")
    # NULL model / reads / mappings / base: refused, nothing dereferenced
    assert lib.phmm_full_prob_reads_copy_num_changes(None, None, None, None, 0, 1, None, None, None, None, None,
                                                     None) == _ffi.PHMM_EINVAL
    assert lib.phmm_full_prob_reads_copy_num_changes(None, None, None, None, 0, 0, None, None, None, None, None,
                                                     None) == _ffi.PHMM_EINVAL


def test_python_binding():
    fn = getattr(D.PHMMModel, "to_full_prob_reads_copy_num_changes", None)
    assert callable(fn)
    assert "posterior.rs:483-515" in fn.__doc__
    assert callable(D.copy_num_changes)


def test_copy_num_changes_round_trips():
    rng = np.random.default_rng(4)
    for C, N in ((1, 1), (7, 50), (64, 300), (130, 40)):
        base = rng.integers(0, 4, size=N).astype(np.uint32)
        cands = np.repeat(base[None, :], C, axis=0)
        for c in range(C):
            ix = rng.integers(0, N, size=rng.integers(0, 6))
            cands[c, ix] = rng.integers(0, 5, size=ix.size)
        off, node, cn = D.copy_num_changes(base, cands)
        assert off.dtype == np.uint64 and node.dtype == np.uint32 and cn.dtype == np.uint32
        assert off[0] == 0 and off.size == C + 1 and np.all(np.diff(off.astype(np.int64)) >= 0)
        back = np.repeat(base[None, :], C, axis=0)
        for c in range(C):
            seg = slice(int(off[c]), int(off[c + 1]))
            assert np.all(np.diff(node[seg].astype(np.int64)) > 0)  # ascending, no node twice
            assert np.all(cn[seg] != base[node[seg]])  # only real changes
            back[c, node[seg]] = cn[seg]
        assert np.array_equal(back, cands)
