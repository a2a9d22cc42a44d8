"""Node groups on the phmm_likelihood handle (set_groups / score_group_changes / move_groups / current_groups) are part
of the ABI: declared in the header with these argument lists, exported by the library, bound in Python; and
graph.unitig_groups, which builds the groups of the test and timing graphs, returns the unitig partition.
No GPU needed."""
import ctypes as C
import os
import re

import numpy as np

import dbgphmm_amd as D
from dbgphmm_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLS = {
    "phmm_likelihood_set_groups": ("int", ["phmm_likelihood *lk", "uint32_t n_groups", "const uint64_t *group_off",
                                           "const uint32_t *group_nodes"]),
    "phmm_likelihood_score_group_changes": ("int", ["phmm_likelihood *lk", "uint32_t n_candidates",
                                                    "const uint64_t *change_off", "const uint32_t *change_group",
                                                    "const uint32_t *change_copy_num", "double *out_logp",
                                                    "double *out_total", "uint64_t *out_n_rescored"]),
    "phmm_likelihood_move_groups": ("int", ["phmm_likelihood *lk", "uint64_t n_changes",
                                            "const uint32_t *change_group", "const uint32_t *change_copy_num",
                                            "double *out_total", "uint64_t *out_n_rescored"]),
    "phmm_likelihood_current_groups": ("int", ["const phmm_likelihood *lk", "uint32_t *out_group_copy_nums"]),
}


def test_header_declares_the_group_calls():
    with open(os.path.join(ROOT, "include", "phmm_amd.h")) as f:
        src = f.read()
    assert re.search(r"#define\s+PHMM_GROUP_MIXED\s+0xffffffffu\b", src)
    assert _ffi.PHMM_GROUP_MIXED == 0xFFFFFFFF
    for name, (ret, want) in DECLS.items():
        decl = re.search(ret + r"\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert decl, name + " is not declared"
        args = [" ".join(a.split()) for a in decl.group(1).split(",")]
        assert args == want, (name, args)
        assert name in _ffi.DECLARED_SYMBOLS


def test_library_exports_and_refuses_null():
    lib = _ffi.lib()
    for name in DECLS:
        assert hasattr(lib, name), name
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    cn = np.ones(4, np.uint32)
    off = np.array([0, 1], np.uint64)
    sentinel = np.full(2, 7.0)
    nout = np.full(2, 9, np.uint64)
    gout = np.full(4, 5, np.uint32)
    assert lib.phmm_likelihood_set_groups(None, 1, p(off), p(cn)) == _ffi.PHMM_EINVAL
    assert lib.phmm_likelihood_set_groups(None, 0, None, None) == _ffi.PHMM_EINVAL
    assert lib.phmm_likelihood_score_group_changes(None, 1, p(off), p(cn), p(cn), None, p(sentinel),
                                                   p(nout)) == _ffi.PHMM_EINVAL
    assert lib.phmm_likelihood_score_group_changes(None, 0, None, None, None, None, None, None) == _ffi.PHMM_EINVAL
    assert lib.phmm_likelihood_move_groups(None, 1, p(cn), p(cn), p(sentinel), p(nout)) == _ffi.PHMM_EINVAL
    assert lib.phmm_likelihood_move_groups(None, 0, None, None, None, None) == _ffi.PHMM_EINVAL
    assert lib.phmm_likelihood_current_groups(None, p(gout)) == _ffi.PHMM_EINVAL
    assert np.all(sentinel == 7.0) and np.all(nout == 9) and np.all(gout == 5) and np.all(cn == 1)
    assert b"NULL" in lib.phmm_last_error()


def test_python_binding():
    for name in ("set_groups", "score_group_changes", "move_groups", "current_groups"):
        fn = getattr(D.Likelihood, name, None)
        assert callable(fn), name
        assert "multi_dbg.rs:1041-1052" in fn.__doc__ or "posterior.rs" in fn.__doc__, name
    assert "multi_dbg.rs:1041-1052" in D.Likelihood.set_groups.__doc__
    assert "posterior.rs:470-528" in D.Likelihood.score_group_changes.__doc__
    assert "posterior.rs:532-600" in D.Likelihood.move_groups.__doc__
    assert "multi_dbg.rs:1041-1052" in D.Likelihood.move_groups.__doc__
    assert "multi_dbg.rs:1041-1052" in D.Likelihood.current_groups.__doc__
    assert callable(D.unitig_groups) and D.unitig_groups is D.graph.unitig_groups


def _diploid():
    """the 12 kb / k = 20 diploid of test_gpu_likelihood.py"""
    hap = D.random_genome(12000, seed=11)
    sg = D.dbg_from_haplotypes([hap, D.diverge(hap, 0.01, seed=12)], 20)
    return sg


def _check_partition(sg):
    off, nodes = D.unitig_groups(sg)
    N = sg.base.size
    assert off.dtype == np.uint64 and nodes.dtype == np.uint32
    off = off.astype(np.int64)
    G = off.size - 1
    # a partition of all N nodes, no empty group
    assert off[0] == 0 and off[-1] == N and np.all(np.diff(off) >= 1)
    assert np.array_equal(np.sort(nodes), np.arange(N))
    src, dst = sg.edge_src.astype(np.int64), sg.edge_dst.astype(np.int64)
    outdeg, indeg = np.bincount(src, minlength=N), np.bincount(dst, minlength=N)
    edges = set(zip(src.tolist(), dst.tolist()))
    cn = sg.copy_num

    def step(a, b):
        return (a, b) in edges and outdeg[a] == 1 and indeg[b] == 1 and cn[a] == cn[b]

    heads, tails = nodes[off[:-1]].astype(np.int64), nodes[off[1:] - 1].astype(np.int64)
    for g in range(G):
        v = nodes[off[g]:off[g + 1]].astype(np.int64)
        # consecutive nodes are joined by an edge with the degree condition; copy numbers constant
        assert all(step(int(a), int(b)) for a, b in zip(v[:-1], v[1:])), g
        assert np.all(cn[v] == cn[v[0]]), g
    # maximal: no tail links to the head of ANOTHER group under the same condition; a tail that links to its own
    # head closes a cycle without a branch, which is cut at its smallest node id
    for g in range(G):
        t = int(tails[g])
        for b in dst[src == t].tolist():
            if step(t, b):
                assert b == int(heads[g]), (g, t, b)
                assert b == int(nodes[off[g]:off[g + 1]].min()), g
    return off, nodes


def test_unitig_groups_diploid():
    sg = _diploid()
    off, nodes = _check_partition(sg)
    sizes = np.diff(off)
    assert 100 <= sizes.size <= 1000 and np.median(sizes) == 20  # (bubble arms of k nodes)
    # groups that hold both n pad nodes and emittable ones exist: the emittable count per group is not its size
    pad = sg.base[nodes] == D.graph.NULL_BASE
    n_pad = np.add.reduceat(pad.astype(np.int64), off[:-1])
    assert np.any((n_pad > 0) & (n_pad < sizes))


def test_unitig_groups_toy_repeat():
    sg, k = D.toy_repeat()
    off, nodes = _check_partition(sg)
    # the copy-number-3 cycle branches where the unique path enters and leaves it: the loop is cut there, not merged
    sizes = np.diff(off)
    assert 2 <= sizes.size < sg.base.size and sizes.max() >= 2
    for g in range(sizes.size):
        assert np.unique(sg.copy_num[nodes[off[g]:off[g + 1]]]).size == 1


def test_unitig_groups_plain_cycle():
    """a cycle without a branch is one group cut at its smallest node id; copy numbers split a path"""
    ring = D.SeqGraph(np.full(5, 2, dtype=np.int64), np.frombuffer(b"ACGTA", dtype=np.uint8).copy(),
                      np.array([3, 4, 0, 1, 2], dtype=np.uint32), np.array([4, 0, 1, 2, 3], dtype=np.uint32), None)
    off, nodes = _check_partition(ring)
    assert off.tolist() == [0, 5] and nodes.tolist() == [0, 1, 2, 3, 4]
    line = D.SeqGraph(np.array([1, 1, 2, 2, 2], dtype=np.int64), np.frombuffer(b"ACGTA", dtype=np.uint8).copy(),
                      np.array([0, 1, 2, 3], dtype=np.uint32), np.array([1, 2, 3, 4], dtype=np.uint32), None)
    off, nodes = _check_partition(line)
    assert off.tolist() == [0, 2, 5] and nodes.tolist() == [0, 1, 2, 3, 4]
