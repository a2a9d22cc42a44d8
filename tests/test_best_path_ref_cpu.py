"""CPU: the Python reference of the best path over mapping lists (tests/best_path_ref.py) stands on its own before it
judges a kernel: against a brute-force enumeration of every state path on a 3-node graph, against the reference's
forward known answer on the linear mock (one path only, so max = sum), and on every case of tests/test_gpu_best_path.py
against the oracle's forward total over the same lists (the best path is one term of that sum) and against score_path,
which re-scores the returned path term by term.  The lists of the shared cases are the oracle's generate_mappings here
(the GPU tests take the GPU's own)."""
import itertools
import json
import math
import os

import numpy as np
import pytest

import dbgphmm_amd as D
import best_path_ref as B
from graph_cases import base_case, with_gaps

KAT = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "kat_hmmv2.json")))
NINF = -math.inf


# ---------------------------------------------------------------- brute force on a 3-node graph
def tiny_model(gaps):
    """0 -> 1 -> 2, 0 -> 2, 1 -> 1: a branch, a skip and a self-loop; rows and init unnormalised, all rates different"""
    p = D.PHMMParams.new(0.07, 0.11, 0.23, 0.01, 40, 50).with_(n_max_gaps=gaps)
    ln = math.log
    return D.PHMMArrays(p, np.frombuffer(b"ACA", dtype=np.uint8).copy(), np.array([ln(0.5), ln(0.3), ln(0.15)]),
                        np.array([0, 1, 0, 1], np.uint32), np.array([1, 2, 2, 1], np.uint32),
                        np.array([ln(0.6), ln(0.7), ln(0.35), ln(0.25)]))


def brute_force(arrays, read, lists):
    """the maximum of score_path over EVERY sequence of rows: per base an emitting state (Match or Ins of a listed slot,
    or InsBegin) and 0 .. G + 1 Del slots; illegal ones are what score_path refuses"""
    G = int(arrays.param.n_max_gaps)
    per_base = []
    for lst in lists:
        n = len(lst)
        emit = [B.INS_BEGIN] + [(s << 2) | k for s in range(n) for k in (0, 1)]
        dels = [c for t in range(G + 2) for c in itertools.product([(s << 2) | 2 for s in range(n)], repeat=t)]
        per_base.append([[e] + list(d) + [B.NONE] * (G + 1 - len(d)) for e in emit for d in dels])
    best, n_paths = NINF, 0
    for rows in itertools.product(*per_base):
        try:
            v, _, _ = B.score_path(arrays, read, lists, np.array(rows, dtype=np.uint32))
        except B.IllegalPath:
            continue
        n_paths += 1
        best = max(best, v)
    return best, n_paths


@pytest.mark.parametrize("gaps", [0, 1])
@pytest.mark.parametrize("read", [b"ACA", b"CAT"])
def test_reference_equals_brute_force(gaps, read):
    arrays = tiny_model(gaps)
    lists = [[0, 1], [2, 1], [1, 2]]
    want, n_paths = brute_force(arrays, read, lists)
    got, rows = B.best_path_ref(arrays, read, lists)
    v, n_terms, _ = B.score_path(arrays, read, lists, rows)
    print(f"G={gaps} {read}: {n_paths} legal paths, best {want:.12f}, reference {got:.12f}")
    assert n_paths > 100
    assert abs(got - want) <= B.bar(n_terms, want) and abs(v - got) <= B.bar(n_terms, want)


def test_score_path_refuses_illegal_paths():
    arrays = tiny_model(1)
    read, lists = b"ACA", [[0, 1, 2], [2, 1, 0], [1, 2]]
    N = B.NONE

    def rows(*r):
        return np.array(r, dtype=np.uint32)
    ok = rows([0 << 2, N, N], [1 << 2, N, N], [1 << 2, N, N])  # M0, M1, M2
    assert B.score_path(arrays, read, lists, ok)[2] == [3, 0, 0, 0]
    bad = {
        "a slot outside its list": rows([0 << 2, N, N], [1 << 2, N, N], [2 << 2, N, N]),
        "a Match with no edge from the previous node": rows([2 << 2, N, N], [1 << 2, N, N], [1 << 2, N, N]),  # M2, M1
        "a Del with no edge from the state before it": rows([0 << 2, N, N], [1 << 2, (2 << 2) | 2, N], [1 << 2, N, N]),  # M1, D0
        "more than G + 1 Dels in a row": np.array([[0, N, N, N], [4, 6, 6, 6], [4, N, N, N]], dtype=np.uint32),
        "an Ins on another node": rows([0 << 2, N, N], [(0 << 2) | 1, N, N], [1 << 2, N, N]),  # M0, I2
        "InsBegin after a node state": rows([0 << 2, N, N], [B.INS_BEGIN, N, N], [1 << 2, N, N]),
        "rows not ending in padding": rows([0 << 2, N, N], [1 << 2, N, (1 << 2) | 2], [1 << 2, N, N]),
        "never leaves InsBegin": rows([B.INS_BEGIN, N, N], [B.INS_BEGIN, N, N], [B.INS_BEGIN, N, N]),
    }
    for what, r in bad.items():
        print(what)
        with pytest.raises(B.IllegalPath):
            B.score_path(arrays, read, lists, r)


# ---------------------------------------------------------------- the linear mock
def test_linear_mock_known_answers():
    a0 = B.linear(0.0)
    best, rows = B.best_path_ref(a0, b"CGATC", B.full_lists(a0, b"CGATC"))
    assert abs(best - KAT["forward_zero_error"]["t4_e"]) <= 1e-5
    assert rows[:, 0].tolist() == [v << 2 for v in range(3, 8)] and np.all(rows[:, 1:] == B.NONE)
    best, rows = B.best_path_ref(a0, b"CGATT", B.full_lists(a0, b"CGATT"))
    assert best == NINF and np.all(rows == B.NONE)
    a1 = B.linear(0.01)
    read = b"ATTCGTCGT"  # freq.rs:499-514: one deletion
    best, rows = B.best_path_ref(a1, read, B.full_lists(a1, read))
    assert rows[:, 0].tolist() == [v << 2 for v in (0, 1, 2, 3, 4, 6, 7, 8, 9)]
    assert rows[4].tolist()[:3] == [4 << 2, (5 << 2) | 2, B.NONE] and np.all(np.delete(rows, 4, 0)[:, 1:] == B.NONE)
    assert B.score_path(a1, read, B.full_lists(a1, read), rows)[2] == [9, 0, 0, 1]
    read = b"ATTCGCATCGT"
    best, rows = B.best_path_ref(a1, read, B.full_lists(a1, read))
    assert rows[5, 0] == (4 << 2) | 1 and B.score_path(a1, read, B.full_lists(a1, read), rows)[2] == [10, 0, 1, 0]
    assert B.best_path_ref(a1, b"", [])[0] == NINF


# ---------------------------------------------------------------- every case of the GPU tests
def _hold_to_oracle(oracle, arrays, reads, po=None, nd=None):
    om = oracle.Model(arrays)
    if po is None:
        (po, nd, _), _ = om.generate_mappings(reads, None, True, n_threads=8)
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])])
    gap = 0.0
    for j, r in enumerate(reads):
        lists = B.lists_of(po, nd, off[j], off[j + 1])
        best, rows = B.best_path_ref(arrays, r, lists)
        total = om.run_with_mapping(r, oracle.Mapping.from_lists(lists)).to_full_prob_forward()
        assert best <= total + 1e-9, (j, best, total)
        if best > NINF:
            v, n_terms, _ = B.score_path(arrays, r, lists, rows)
            assert abs(v - best) <= B.bar(n_terms, best), (j, v, best)
            gap = max(gap, total - best)
    return gap, po, nd


def test_linear_mock_cases(oracle):
    for p, read in ((0.0, b"CGATC"), (0.0, b"CGATT"), (0.01, b"ATTCGTCGT"), (0.01, b"ATTCGCATCGT"), (0.01, b"ATTCGATGGT")):
        a = B.linear(p)
        full = B.full_lists(a, read)
        po = np.arange(len(read) + 1, dtype=np.uint64) * a.n_nodes
        _hold_to_oracle(oracle, a, [read], po, np.array(sum(full, []), dtype=np.uint32))
        if p > 0.0:
            _hold_to_oracle(oracle, a, [read])


@pytest.mark.parametrize("graph", ["dbg", "zoo", "zoo_lean"])
def test_graph_cases(oracle, graph):
    b = base_case(graph)
    gap, _, _ = _hold_to_oracle(oracle, b["arrays"], b["reads"])
    print(f"{graph}: largest ln P(forward) - ln P(best path) {gap:.3f}")


def test_fuzz_cases(oracle):
    for c in B.fuzz_cases():
        gap, _, _ = _hold_to_oracle(oracle, c["arrays"], c["reads"])
        print(f"{c['tag']}: largest gap {gap:.3f}")


def test_del_level_cases(oracle):
    arrays, read = B.two_deletions()
    for gaps in (0, 4, 6):
        a = with_gaps(arrays, gaps)
        _, po, nd = _hold_to_oracle(oracle, a, [read])
        _, rows = B.best_path_ref(a, read, B.lists_of(po, nd, 0, len(read)))
        dels = (rows[:, 1:] != B.NONE).sum(axis=1)
        assert rows.shape[1] == gaps + 2 and dels.sum() == 2
        assert dels.max() == (1 if gaps == 0 else 2)  # the read does carry two adjacent deletions


@pytest.mark.parametrize("width", B.WIDTHS)
def test_width_cases(oracle, width):
    arrays, reads = B.width_reads(width)
    assert 1 < len(reads) and all(30 < len(r) <= 200 for r in reads)
    (po, nd, _), _ = oracle.Model(arrays).generate_mappings(reads, None, True, n_threads=8)
    ppo, pnd = B.pad_lists(po, nd, reads, arrays.n_nodes, width)
    assert int(np.diff(ppo.astype(np.int64)).max()) == width
    _hold_to_oracle(oracle, arrays, reads, ppo, pnd)


def test_long_read_case(oracle):
    arrays, read = B.long_read()
    assert len(read) == 3000
    _hold_to_oracle(oracle, arrays, [read])
