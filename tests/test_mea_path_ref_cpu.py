"""CPU: the Python restatement of the weighted walk over mapping lists (tests/mea_path_ref.py) stands on its own before
it judges a kernel.  On the tiny models of test_best_path_ref_cpu.py a brute force over every legal path, from the model
alone, gives the score (the largest left-to-right weight sum) and, with dyadic weights whose sums are exact, the path the
tie rule of include/phmm_amd_path.h leaves: the lexicographically first optimum under that file's tie_key.  Hand cases
pin one admissibility clause of include/phmm_amd_mea.h each."""
import math

import numpy as np
import pytest

import dbgphmm_amd as D
import best_path_ref as B
import mea_path_ref as M
from test_best_path_ref_cpu import _tiny_int, legal_paths, random_int_case, tie_key, tiny_model

NINF = -math.inf
N_ = B.NONE
N_RANDOM = 70


def _continues_from_first_entries(lists, rows):
    """"a node listed twice is looked up at its first entry": a state on a later entry of its node may end the path, but
    nothing continues from it.  Under the best path such a state has the value of the first entry's, so the rule costs
    nothing there; here the two entries carry weights of their own, and the rule decides which paths exist."""
    states = [(pos, c >> 2) for pos, row in enumerate(rows) for c in row if c not in (B.NONE, B.INS_BEGIN)]
    return all(lists[pos].index(lists[pos][s]) == s for pos, s in states[:-1])


def _admissible(arrays, read, lists):
    """every legal path whose every transition and emission has probability > 0, as rows"""
    out = []
    for rows in legal_paths(arrays, len(read), lists):
        if not _continues_from_first_entries(lists, rows):
            continue
        rows = np.array(rows, dtype=np.uint32)
        if B.score_path(arrays, read, lists, rows)[0] > NINF:
            out.append(rows)
    return out


def _brute(arrays, read, lists, w, ib=None):
    """-> (score, rows of the lexicographically first optimum or None, paths, optima)"""
    scored = [(M.score_rows(arrays, read, lists, rows, w, ib)[0], rows) for rows in _admissible(arrays, read, lists)]
    best = max([v for v, _ in scored], default=NINF)
    if best == NINF:
        return NINF, None, len(scored), 0
    optima = [rows for v, rows in scored if v == best]
    return best, min(optima, key=tie_key), len(scored), len(optima)


def _n_entries(lists):
    return sum(len(x) for x in lists)


def _check(arrays, read, lists, w, ib, rows_too=True):
    want, rows, n_paths, optima = _brute(arrays, read, lists, w, ib)
    got, got_rows = M.weighted_path_ref(arrays, read, lists, w, ib)
    assert got == want, (got, want)
    if want == NINF:
        assert np.all(got_rows == B.NONE)
    elif rows_too:
        assert np.array_equal(got_rows, rows), (n_paths, optima, got_rows.tolist(), rows.tolist())
    else:
        assert M.score_rows(arrays, read, lists, got_rows, w, ib)[0] == want
    return want, optima


@pytest.mark.parametrize("kind", ["dyadic", "zeros"])
def test_restatement_returns_the_lexicographically_first_optimum(kind):
    """dyadic weights (multiples of 2^-10: every sum is exact) and all-zero weights (the tie rule alone)"""
    finite = ties = 0
    for seed in range(N_RANDOM):
        arrays, read, lists = random_int_case(seed)
        rng = np.random.default_rng([20261101, seed])
        n = _n_entries(lists)
        w = M.dyadic(rng, (n, 3)) if kind == "dyadic" else np.zeros((n, 3))
        ib = M.dyadic(rng, len(read)) if kind == "dyadic" and seed % 2 else None
        want, optima = _check(arrays, read, lists, w, ib)
        finite += want > NINF
        ties += optima > 1
        if kind == "zeros" and want > NINF:
            assert want == 0.0
    print(f"{kind}: {finite} of {N_RANDOM} cases have a path, {ties} of them more than one optimal path")
    assert finite >= 40 and ties >= (20 if kind == "zeros" else 5)


def test_arbitrary_doubles_equal_the_brute_force_maximum():
    """rounding is monotone: the recursion's maximum is the maximum of the left-to-right sums, exactly"""
    finite = 0
    for seed in range(N_RANDOM):
        arrays, read, lists = random_int_case(seed)
        rng = np.random.default_rng([20261102, seed])
        w = rng.normal(size=(_n_entries(lists), 3)) * 10.0 ** rng.integers(-3, 4, size=(_n_entries(lists), 3))
        ib = rng.normal(size=len(read))
        want, _ = _check(arrays, read, lists, w, ib, rows_too=False)
        finite += want > NINF
    assert finite >= 40
    for gaps in (0, 1):  # ordinary logs: every structurally legal path is admissible
        arrays, lists = tiny_model(gaps), [[0, 1], [2, 1], [1, 2]]
        rng = np.random.default_rng([20261103, gaps])
        for read in (b"ACA", b"CAT"):
            w = rng.normal(size=(6, 3))
            assert len(_admissible(arrays, read, lists)) > 100
            _check(arrays, read, lists, w, rng.normal(size=3), rows_too=False)


def test_negative_weights():
    """all weights negative: the path with the fewest, lightest states wins, and no state is taken for free"""
    for seed in range(20):
        arrays, read, lists = random_int_case(seed)
        rng = np.random.default_rng([20261104, seed])
        w = -1.0 - M.dyadic(rng, (_n_entries(lists), 3), 0, 16)
        want, _ = _check(arrays, read, lists, w, -1.0 - M.dyadic(rng, len(read), 0, 16))
        assert want == NINF or want < 0.0


def _w(lists, **named):
    """zeros but for named entries 'p<pos>s<slot>k<kind>' = weight"""
    w = np.zeros((_n_entries(lists), 3))
    off = M.entry_offsets(lists)
    for name, v in named.items():
        pos, rest = name[1:].split("s")
        s, k = rest.split("k")
        w[off[int(pos)] + int(s), int(k)] = v
    return w


def test_mismatch_of_probability_zero_bars_the_match():
    """read AC on 0 -> 1 (bases A, C): the heavy Match of node 0 at base 1 mismatches; with p_mismatch = -inf it is out"""
    lists = [[0, 1], [0, 1]]
    w = _w(lists, p1s0k0=100.0, p1s1k0=1.0)
    open_ = _tiny_int(0, [-1, -1, -1], [0, 0, 0, 0])
    s, rows = M.weighted_path_ref(open_, b"AC", lists, w)
    assert s == 100.0 and rows[1, 0] == (0 << 2) | 0  # InsBegin, then Match on node 0
    barred = _tiny_int(0, [-1, -1, -1], [0, 0, 0, 0], p_mismatch=NINF)
    s, rows = M.weighted_path_ref(barred, b"AC", lists, w)
    assert s == 1.0 and rows.tolist() == [[0 << 2, N_], [1 << 2, N_]]
    _check(open_, b"AC", lists, w, None)
    _check(barred, b"AC", lists, w, None)


def test_no_end_no_path():
    a = _tiny_int(1, [-1, -1, -1], [0, 0, 0, 0], p_end=NINF)
    lists = [[0, 1], [1, 2]]
    s, rows = M.weighted_path_ref(a, b"AC", lists, np.ones((4, 3)))
    assert s == NINF and np.all(rows == N_)
    with pytest.raises(B.IllegalPath):
        M.score_rows(a, b"AC", lists, np.array([[0, N_, N_], [0, N_, N_]], dtype=np.uint32), np.ones((4, 3)))
    assert M.weighted_path_ref(_tiny_int(1, [-1, -1, -1], [0, 0, 0, 0]), b"", [], np.zeros((0, 3)))[0] == NINF


def test_an_edge_of_probability_zero_is_no_edge():
    """0 -> 2 carries the weight but has t = -inf: the path goes 0 -> 1 instead; with it open, 0 -> 2"""
    lists = [[0], [2, 1]]
    w = _w(lists, p1s0k0=5.0, p1s1k0=1.0, p1s0k2=-1.0)  # (the Del weight: no free Del on 2 behind the Match on 1)
    shut = _tiny_int(0, [-1, NINF, NINF], [0, 0, NINF, 0])
    s, rows = M.weighted_path_ref(shut, b"AC", lists, w)
    assert s == 1.0 and rows.tolist() == [[0, N_], [1 << 2, N_]]
    s, rows = M.weighted_path_ref(_tiny_int(0, [-1, NINF, NINF], [0, 0, 0, 0]), b"AC", lists, w)
    assert s == 5.0 and rows.tolist() == [[0, N_], [0 << 2, N_]]
    _check(shut, b"AC", lists, w, None)
    # init = -inf on the node, p_random = -inf: no InsBegin, no Ins
    a = _tiny_int(0, [-1, -1, -1], [0, 0, 0, 0], p_random=NINF)
    s, rows = M.weighted_path_ref(a, b"AC", [[0, 1], [0, 1]], _w([[0, 1], [0, 1]], p1s0k1=50.0), np.full(2, 50.0))
    assert s == 0.0 and not np.any(rows[:, 0] == B.INS_BEGIN) and not np.any(rows[:, 0] & 3 == 1)
    _check(a, b"AC", [[0, 1], [0, 1]], _w([[0, 1], [0, 1]], p1s0k1=50.0), np.full(2, 50.0))


def test_ib_weight_makes_ins_begin_win():
    a = _tiny_int(0, [-1, -1, -1], [0, 0, 0, 0])
    lists = [[0, 1], [0, 1], [1, 2]]
    w = np.ones((6, 3))
    s, rows = M.weighted_path_ref(a, b"ACA", lists, w)
    assert not np.any(rows == B.INS_BEGIN)
    ib = np.array([10.0, 10.0, 10.0])
    s, rows = M.weighted_path_ref(a, b"ACA", lists, w, ib)
    assert rows[:, 0].tolist() == [B.INS_BEGIN] * 3 and rows[2, 1] & 3 == 2  # (a Del behind the last base leaves InsBegin)
    assert s == M.score_rows(a, b"ACA", lists, rows, w, ib)[0] == 31.0
    _check(a, b"ACA", lists, w, ib)


def test_del_levels_share_one_weight_and_resolve_to_the_lower():
    """the free-Del graph of the best path's hand case: Del on 2 is reached at level 0 (0 -> 2), 1 and 2; all carry the
    entry's Del weight once per state, so the shortest chain to node 2 holds the maximum when the other Dels weigh 0"""
    a = _tiny_int(2, [-1, NINF, NINF], [0, 0, 0, 0])
    lists = [[2, 1, 0]]
    w = _w(lists, p0s0k2=3.0)
    s, rows = M.weighted_path_ref(a, b"A", lists, w)
    assert s == 3.0 and rows.tolist() == [[(2 << 2) | 0, (0 << 2) | 2, N_, N_]]
    _check(a, b"A", lists, w, None)
    w = _w(lists, p0s0k2=3.0, p0s1k2=1.0)  # a Del on 1 in between pays: 0 -> 1 -> 1 -> 2
    s, rows = M.weighted_path_ref(a, b"A", lists, w)
    assert s == 5.0 and rows.tolist() == [[(2 << 2) | 0, (1 << 2) | 2, (1 << 2) | 2, (0 << 2) | 2]]
    _check(a, b"A", lists, w, None)


def test_score_rows_sums_in_path_order():
    a = tiny_model(1)
    lists = [[0, 1], [2, 1], [1, 2]]
    w = np.array([[1e16, 0, 0], [0, 0, 1.0], [0, 0, 0], [1.0, 0, 0], [0, 0, 0], [-1e16, 0, 0]])
    rows = np.array([[0 << 2, (1 << 2) | 2, N_], [1 << 2, N_, N_], [1 << 2, N_, N_]], dtype=np.uint32)  # M0, D1, M1, M2
    got, counts = M.score_rows(a, b"ACA", lists, rows, w)
    assert got == ((1e16 + 1.0) + 1.0) + -1e16 == 0.0 and counts == [3, 0, 0, 1]  # (right to left it would be 2)
    assert M.counts_of(a, b"ACA", lists, rows) == counts
