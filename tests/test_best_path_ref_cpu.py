"""CPU: the Python reference of the best path over mapping lists (tests/best_path_ref.py) stands on its own before it
judges a kernel: against a brute-force enumeration of every state path on a 3-node graph, against the reference's
forward known answer on the linear mock (one path only, so max = sum), and on every case of tests/test_gpu_best_path.py
against the oracle's forward total over the same lists (the best path is one term of that sum) and against score_path,
which re-scores the returned path term by term.  The lists of the shared cases are the oracle's generate_mappings here
(the GPU tests take the GPU's own).

The GPU tests hold the kernel to this reference exactly, rows included, so its tie rule is pinned here without its own
code: a brute force over every path of small integer-log models picks the lexicographically first optimum under the
ranks of include/phmm_amd_path.h, and hand-checked cases add one clause each.  The odd-list and integer-log cases the
GPU tests run are counted here: which path forms the reference's paths show, how many have a path, and why the others
have none."""
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


# ---------------------------------------------------------------- the tie rule, pinned without best_path_ref
# Integer logs make every path value exact, so "equal" means equal and, in exact arithmetic, every prefix of an optimal
# path is optimal for the state it ends in.  The local rule of the header (each maximum keeps the lowest rank among equal
# candidates, and the walk back follows what was kept) then returns the optimal path whose decisions, listed in the order
# the walk back meets them, are lexicographically smallest.  tie_key writes that list down from the TIES paragraph of
# include/phmm_amd_path.h; legal_paths enumerates the paths from the model alone.
_LAST = 1 << 30  # Begin / InsBegin: behind every node state


def tie_key(rows):
    rows = [[c for c in row if c != B.NONE] for row in np.asarray(rows).tolist()]
    key = [rows[-1][-1]]  # the end state: (slot << 2) | kind
    for p in range(len(rows) - 1, -1, -1):
        emit, dels = rows[p][0], rows[p][1:]
        if dels:  # the Del the path leaves the column from: its level (the lower first), the parents down the chain by
            #       slot, then the source of level 0 as (slot << 1) | (0 Match, 1 Ins), InsBegin last
            key.append(len(dels) - 1)
            key += [c >> 2 for c in dels[-2::-1]]
            key.append(_LAST if emit == B.INS_BEGIN else ((emit >> 2) << 1) | (emit & 3))
        if emit == B.INS_BEGIN:
            continue  # (InsBegin comes from Begin or InsBegin: nothing to choose)
        before = rows[p - 1][-1] if p else B.INS_BEGIN
        if emit & 3 == 0:  # the source of a Match: (slot << 2) | kind, Begin / InsBegin last
            key.append(_LAST if before == B.INS_BEGIN else before)
        else:  # the source of an Ins: Match, Ins, Del -- of the node's FIRST entry in the list before
            key += [before & 3, before >> 2]
    return key


def legal_paths(arrays, L, lists):
    """every path of the model over the lists, as rows: per base an emitting state and 0 .. G + 1 Dels"""
    G = int(arrays.param.n_max_gaps)
    edges = set(zip(arrays.edge_src.tolist(), arrays.edge_dst.tolist()))

    def chains(pos, kind, node, left):
        yield []
        if left:
            for s, w in enumerate(lists[pos]):
                if kind == "IB" or (node, w) in edges:
                    for rest in chains(pos, "D", w, left - 1):
                        yield [(s << 2) | 2] + rest

    def walk(pos, kind, node):
        if pos == L:
            if kind != "IB":
                yield []
            return
        heads = [(B.INS_BEGIN, "IB", None)] if kind in ("B", "IB") else []
        for s, v in enumerate(lists[pos]):
            if kind in ("B", "IB") or (node, v) in edges:
                heads.append(((s << 2) | 0, "M", v))
            if kind not in ("B", "IB") and v == node:
                heads.append(((s << 2) | 1, "I", v))
        for code, k, v in heads:
            for ch in chains(pos, k, v, G + 1):
                k2, v2 = ("D", lists[pos][ch[-1] >> 2]) if ch else (k, v)
                for rest in walk(pos + 1, k2, v2):
                    yield [[code] + ch + [B.NONE] * (G + 1 - len(ch))] + rest
    return walk(0, "B", None)


def lexicographic_best(arrays, read, lists):
    """-> (best, rows or None, n_paths, n_optima): among the paths whose value is exactly the maximum, the smallest tie_key"""
    scored = [(B.score_path(arrays, read, lists, np.array(rows, dtype=np.uint32))[0], rows)
              for rows in legal_paths(arrays, len(read), lists)]
    best = max([v for v, _ in scored], default=NINF)
    if best == NINF:
        return NINF, None, len(scored), 0
    optima = [rows for v, rows in scored if v == best]
    return best, np.array(min(optima, key=tie_key), dtype=np.uint32), len(scored), len(optima)


def random_int_case(seed):
    """3 nodes, up to 6 edges (one of them twice), every log a small non-positive integer with some -inf, a read of 3
    bases over two letters, lists of 0 to 3 entries (0 to 2 at n_max_gaps = 2, which keeps the enumeration near 1e4 paths; repeats allowed), n_max_gaps = seed % 3"""
    rng = np.random.default_rng([20261022, seed])

    def logs(n, lo, p_inf):
        return np.where(rng.random(n) < p_inf, NINF, rng.choice([0.0, 0.0, -1.0, -2.0][:lo + 2], size=n))  # (0 twice: free steps tie)
    names = ["p_mismatch", "p_match", "p_random", "p_gap_open", "p_gap_ext", "p_end", "p_MM", "p_IM", "p_DM", "p_MI",
             "p_II", "p_DI", "p_MD", "p_ID", "p_DD"]
    p = B.int_params(seed % 3, **dict(zip(names, logs(15, 2, 0.08).tolist())))
    pairs = [(u, v) for u in range(3) for v in range(3)]
    e = [pairs[i] for i in rng.choice(9, size=int(rng.integers(3, 6)), replace=False)]
    e.append(e[0])
    e = np.array(e, dtype=np.uint32)
    arrays = D.PHMMArrays(p, rng.choice(np.frombuffer(b"AC", dtype=np.uint8), size=3), logs(3, 2, 0.2),
                          e[:, 0].copy(), e[:, 1].copy(), logs(len(e), 2, 0.1))
    read = bytes(rng.choice(np.frombuffer(b"AC", dtype=np.uint8), size=3))
    lists = [rng.integers(0, 3, size=min(int(rng.choice([0, 1, 2, 2, 3, 3, 3])), 3 if seed % 3 < 2 else 2)).tolist() for _ in range(3)]
    return arrays, read, lists


def test_legal_paths_are_all_the_paths():
    """the enumeration the tie tests use finds exactly the paths the exhaustive product over rows finds"""
    arrays = tiny_model(1)
    lists = [[0, 1], [2, 1], [1, 2]]
    _, n_paths = brute_force(arrays, b"ACA", lists)
    assert sum(1 for _ in legal_paths(arrays, 3, lists)) == n_paths


N_RANDOM = 70


def test_reference_returns_the_lexicographically_first_optimum():
    finite = ties = 0
    for seed in range(N_RANDOM):
        arrays, read, lists = random_int_case(seed)
        want, rows, n_paths, optima = lexicographic_best(arrays, read, lists)
        got, got_rows = B.best_path_ref(arrays, read, lists)
        assert got == want, (seed, got, want)
        if want == NINF:
            assert np.all(got_rows == B.NONE)
            continue
        finite += 1
        ties += optima > 1
        assert np.array_equal(got_rows, rows), (seed, n_paths, optima, got_rows.tolist(), rows.tolist())
    print(f"{finite} of {N_RANDOM} cases have a path, {ties} of them more than one optimal path")
    assert finite >= 40 and ties >= 20


def _tiny_int(gaps, init, trans, **over):
    """tiny_model's graph (0 -> 1 -> 2, 0 -> 2, 1 -> 1; bases A C A) with integer logs"""
    return D.PHMMArrays(B.int_params(gaps, **over), np.frombuffer(b"ACA", dtype=np.uint8).copy(), np.array(init, dtype=np.float64),
                        np.array([0, 1, 0, 1], np.uint32), np.array([1, 2, 2, 1], np.uint32), np.array(trans, dtype=np.float64))


N_ = B.NONE
HAND_CASES = {
    # M, I and D of entry 0 all end at -3: the end state is the Match
    "Match before Ins before Del": (_tiny_int(0, [-1, -1, -1], [0, 0, 0, 0], p_MM=-1, p_MI=0, p_MD=0, p_ID=0, p_mismatch=-2),
                                    b"CC", [[1], [1]], [[0, N_], [0, N_]]),
    # the second base is a mismatch, so Match is -5 and Ins and Del tie at -3: Ins
    "Ins before Del": (_tiny_int(0, [-1, -1, -1], [0, 0, 0, 0], p_MM=-1, p_MI=0, p_MD=0, p_ID=0, p_mismatch=-2),
                       b"CA", [[1], [1]], [[0, N_], [1, N_]]),
    # init on 0 alone; Del on 2 (slot 0) has the value of Match on 0 at level 0 (0 -> 2), level 1 (0 -> 1 -> 2) and level 2 (.. 1 -> 1 ..)
    "the lower Del level": (_tiny_int(2, [-1, NINF, NINF], [0, 0, 0, 0], p_MD=0, p_DD=0),
                            b"A", [[2, 1, 0]], [[(2 << 2) | 0, (0 << 2) | 2, N_, N_]]),
    # Match on 1 from Match on 0 and from InsBegin both give -2: the node state
    "InsBegin last": (_tiny_int(0, [-1, -1, -1], [-1, 0, 0, 0], p_IM=0, p_MI=0),
                      b"AC", [[0], [1]], [[0, N_], [0, N_]]),
}


def _parallel_edges():
    """2 has the parents 0 (one edge of -2) and 1 (edges of -3 and -1, listed around the other): through 1"""
    a = D.PHMMArrays(B.int_params(0), np.frombuffer(b"AAC", dtype=np.uint8).copy(), np.array([-1.0, -1.0, -1.0]),
                     np.array([1, 0, 1], np.uint32), np.array([2, 2, 2], np.uint32), np.array([-3.0, -2.0, -1.0]))
    return a, b"AC", [[0, 1], [2]], [[(1 << 2) | 0, N_], [0, N_]]


@pytest.mark.parametrize("name", list(HAND_CASES) + ["parallel edges"])
def test_tie_rule_by_hand(name):
    arrays, read, lists, want_rows = _parallel_edges() if name == "parallel edges" else HAND_CASES[name]
    best, rows = B.best_path_ref(arrays, read, lists)
    assert rows.tolist() == want_rows, (best, rows.tolist())
    _, lex, _, _ = lexicographic_best(arrays, read, lists)
    assert lex.tolist() == want_rows
    if name == "parallel edges":
        assert best == -1.0 + 0.0 + 0.0 + (-1.0 + 0.0 + 0.0) + -1.0  # init p_MM match, the edge of -1 p_MM match, p_end


def test_bubble_paths_follow_the_list_order():
    arrays, read, orders = B.bubble_case()
    values = set()
    for name, (order, nodes) in orders.items():
        best, rows = B.best_path_ref(arrays, read, [order] * len(read))
        values.add(best)
        assert [order[c >> 2] for c in rows[:, 0].tolist()] == nodes and np.all(rows[:, 0] & 3 == 0), (name, rows.tolist())
        assert np.all(rows[:, 1:] == B.NONE)
    assert len(values) == 1  # the same double in every order


# ---------------------------------------------------------------- the shared odd-list and integer-log cases
def _features_of(groups):
    tot, n, finite, causes = {}, 0, 0, set()
    for g in groups:
        for read, lists, cause in zip(g["reads"], g["lists"], g["causes"]):
            best, rows = B.best_path_ref(g["arrays"], read, lists)
            n += 1
            if best > NINF:
                finite += 1
                v, n_terms, _ = B.score_path(g["arrays"], read, lists, rows)
                assert abs(v - best) <= B.bar(n_terms, best), (g["tag"], read, v, best)
                assert rows.shape == (len(read), g["arrays"].param.n_max_gaps + 2)
            else:
                assert np.all(rows == B.NONE)
                assert cause is not None, (g["tag"], read, lists)  # a read without a path says why
                causes.add(cause)
            for k, c in B.features(rows).items():
                tot[k] = tot.get(k, 0) + c
    return tot, n, finite, causes


def _int_groups():
    return [dict(tag=f"integer-log {g}", arrays=c["arrays"], reads=c["reads"], lists=c["lists"], causes=[None] * len(c["reads"]))
            for g, c in ((g, B.int_case(g)) for g in ("zoo", "dbg"))]


def test_shared_cases_cover_every_path_form(oracle):
    tot = {}
    causes = set()
    for family, groups in (("odd lists, ordinary logs", B.odd_cases("ord")), ("odd lists, integer logs", B.odd_cases("int")),
                           ("integer-log zoo and dbg", _int_groups())):
        t, n, finite, c = _features_of(groups)
        print(f"{family}: {n} reads, {finite} with a path; " + ", ".join(f"{k} {t.get(k, 0)}" for k in B.FEATURES))
        assert 2 * finite >= n, family
        causes |= c
        for k, v in t.items():
            tot[k] = tot.get(k, 0) + v
    print("together: " + ", ".join(f"{k} {tot.get(k, 0)}" for k in B.FEATURES))
    assert all(tot.get(k, 0) >= 3 for k in B.FEATURES), tot
    assert set(tot) <= set(B.FEATURES), tot  # (no transition outside the model)
    assert causes == {"empty last list", "-inf parameters", "unreachable start"}


@pytest.mark.parametrize("graph", ["zoo", "dbg"])
def test_integer_log_cases_have_ties(oracle, graph):
    """reversing every list changes at least one path and no value; lists stay in the <= 64 class, reads at 40 bases"""
    c = B.int_case(graph)
    a = c["arrays"]
    assert all(len(r) <= 40 for r in c["reads"]) and len(c["reads"]) == 12
    assert all(20 <= len(lst) <= 60 and max(lst) < c["n_real"] for per in c["lists"] for lst in per)
    assert a.n_nodes == c["n_real"] + B.N_ISOLATED and not np.isfinite(a.init_logp[c["n_real"]:]).any()
    assert not (np.isin(a.edge_src, np.arange(c["n_real"], a.n_nodes)) | np.isin(a.edge_dst, np.arange(c["n_real"], a.n_nodes))).any()
    differ = 0
    for read, lists, rev in zip(c["reads"], c["lists"], B.reversed_lists(c["lists"])):
        best, rows = B.best_path_ref(a, read, lists)
        best2, rows2 = B.best_path_ref(a, read, rev)
        assert best == best2 and best == round(best) and best > NINF
        nodes = [[lists[g][c_ >> 2] for c_ in row if c_ != B.NONE and c_ != B.INS_BEGIN] for g, row in enumerate(rows.tolist())]
        nodes2 = [[rev[g][c_ >> 2] for c_ in row if c_ != B.NONE and c_ != B.INS_BEGIN] for g, row in enumerate(rows2.tolist())]
        differ += nodes != nodes2
    print(f"integer-log {graph}: {differ} of 12 paths change when every list is reversed")
    assert differ >= 1


def test_unreachable_padding_changes_nothing():
    """lists padded with isolated nodes, behind or in front: the same value, the same path with the slots shifted"""
    c = B.int_case("zoo")
    a = c["arrays"]
    for read, lists in list(zip(c["reads"], c["lists"]))[:2]:
        best, rows = B.best_path_ref(a, read, lists)
        for width, front in ((65, False), (400, False), (400, True)):
            padded = B.pad_unreachable(lists, c["n_real"], width, front)
            assert all(len(lst) == width for lst in padded)
            best2, rows2 = B.best_path_ref(a, read, padded)
            assert best2 == best and np.array_equal(rows2, B.shift_slots(rows, lists, width) if front else rows)
    assert int((B.shift_slots(rows, lists, 400)[:, 0] >> 2).max()) > 255  # slots that need the 9th bit


def test_many_short_reads_case():
    arrays, reads, lists = B.many_short_reads()
    assert len(reads) >= 300 and all(1 <= len(r) <= 12 for r in reads) and max(len(x) for per in lists for x in per) <= 8
    assert sorted(set(len(r) for r in reads)) == list(range(1, 13))
    finite = sum(B.best_path_ref(arrays, r, l)[0] > NINF for r, l in zip(reads, lists))
    assert 2 * finite >= len(reads)


# ---------------------------------------------------------------- path_states on InsBegin rows
def test_path_states_with_ins_begin_rows():
    """a hand-written path: InsBegin twice, a Del behind the second InsBegin, Match, Ins, Match with two Dels"""
    from types import SimpleNamespace
    lists = [[7, 3], [3, 5], [5, 6, 3], [6], [9, 8, 6]]
    po, nd = B.csr([[[1, 2]], lists])  # (read 1 of two: its rows start at base 1)
    mp = SimpleNamespace(arrays=lambda: (po, nd, None), reads=SimpleNamespace(offsets=np.array([0, 1, 6], dtype=np.uint64)))
    N, IBEG = B.NONE, B.INS_BEGIN
    path = np.array([[(1 << 2) | 0, N, N, N],
                     [IBEG, N, N, N], [IBEG, (1 << 2) | 2, N, N], [(1 << 2) | 0, N, N, N], [(0 << 2) | 1, N, N, N],
                     [(2 << 2) | 0, (1 << 2) | 2, (0 << 2) | 2, N]], dtype=np.uint32)
    assert D.path_states(mp, 1, path) == [(None, "IB"), (None, "IB"), (5, "D"), (6, "M"), (6, "I"), (6, "M"), (8, "D"), (9, "D")]
    assert D.path_states(mp, 0, path) == [(2, "M")]
    assert D.path_states(mp, 1, np.full((6, 4), N, dtype=np.uint32)) == []
