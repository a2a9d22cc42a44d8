"""CPU: the Python restatement of the alignment records (tests/alignments_ref.py) stands on its own before it judges a
kernel.  Round trip: on the best paths of best_path_ref over the odd-list reads, the many short reads, the bubble case
and the two-deletions read, expand(compress(rows)) is the (node, kind) sequence the rows themselves spell, and the three
invariants of include/phmm_amd_align.h hold.  Hand-written records pin one clause of the header each.  The host classes
that read records (dbgphmm_amd.Alignments, dbgphmm_amd.formats) are held to the restatement here as well."""
import io
import math

import numpy as np
import pytest

import dbgphmm_amd as D
import alignments_ref as A
import best_path_ref as B
from graph_cases import with_gaps

NONE, IB = A.NONE, A.INS_BEGIN


def _round_trip(arrays, read, lists):
    """-> (record, has a path)"""
    best, rows = B.best_path_ref(arrays, read, lists)
    rec = A.compress(arrays, read, lists, rows)
    want = A.states_of_rows(lists, rows)
    assert A.expand(*rec) == want
    counts = B.score_path(arrays, read, lists, rows)[2] if best > -math.inf else [0, 0, 0, 0]
    A.check_invariants(*rec, len(read), counts)
    if best == -math.inf:
        assert rec == ([], [], [])
    return rec, best > -math.inf


@pytest.mark.parametrize("flavour", ["ord", "int"])
def test_round_trip_odd_lists(flavour):
    n = with_path = 0
    for g in B.odd_cases(flavour):
        for read, lists in zip(g["reads"], g["lists"]):
            with_path += _round_trip(g["arrays"], read, lists)[1]
            n += 1
    assert n == 213 and 0 < with_path < n


def test_round_trip_many_short_reads():
    arrays, reads, lists = B.many_short_reads()
    assert len(reads) == 320
    ops = set()
    for read, ls in zip(reads, lists):
        rec, _ = _round_trip(arrays, read, ls)
        ops |= {w & 15 for w in rec[0]}
    assert ops == {A.INS, A.DEL, A.EQ, A.DIFF}  # (every op occurs somewhere)


def test_round_trip_bubble_and_two_deletions():
    arrays, read, orders = B.bubble_case()
    for name, (order, nodes) in orders.items():
        rec, ok = _round_trip(arrays, read, [order] * len(read))
        assert ok and A.expand(*rec) == [(v, "M") for v in nodes]
    assert A.compress(arrays, read, [orders["ascending"][0]] * 5, B.best_path_ref(arrays, read, [orders["ascending"][0]] * 5)[1]) \
        == ([(5 << 4) | A.EQ], [0, 3, 6], [2, 2, 1])  # nodes 0 1 3 4 6
    arrays, read = B.two_deletions()
    for gaps in (0, 4):
        a = with_gaps(arrays, gaps)
        from oracle import oracle as O
        O.build()
        (po, nd, _), _ = O.Model(a).generate_mappings([read], None, True, n_threads=4)
        lists = B.lists_of(po, nd, 0, len(read))
        rec, ok = _round_trip(a, read, lists)
        assert ok and A.op_totals(rec[0])[3] == 2
        if gaps:
            assert (2 << 4) | A.DEL in rec[0]  # the two Dels stand in one row: one CIGAR run of 2


# ---------------------------------------------------------------- hand-written records, one per clause
def _linear(n=8, gaps=2, bases=b"ACGTACGT"):
    """a chain 0 -> 1 -> .. with the given bases (only the emissions and n_max_gaps matter to compress)"""
    p = D.PHMMParams.uniform(0.01).with_(n_max_gaps=gaps)
    return D.PHMMArrays(p, np.frombuffer(bases[:n], dtype=np.uint8).copy(), np.full(n, math.log(1.0 / n)),
                        np.arange(n - 1, dtype=np.uint32), np.arange(1, n, dtype=np.uint32), np.zeros(n - 1))


def _rows(stride, *rows):
    return np.array([list(r) + [NONE] * (stride - len(r)) for r in rows], dtype=np.uint32)


def M(s):
    return (s << 2) | 0


def I(s):  # noqa: E743
    return (s << 2) | 1


def Dl(s):
    return (s << 2) | 2


FULL = list(range(8))


def _case(read, rows, lists=None, gaps=2, arrays=None):
    a = arrays or _linear(gaps=gaps)
    lists = lists or [FULL] * len(read)
    rec = A.compress(a, read, lists, _rows(gaps + 2, *rows))
    assert A.expand(*rec) == A.states_of_rows(lists, _rows(gaps + 2, *rows))
    A.check_invariants(*rec, len(read))
    return rec


def test_clause_ins_begin_prefix():
    # T, T put in front of A C on nodes 0 1: an I before the first step is InsBegin
    rec = _case(b"TTAC", [[IB], [IB], [M(0)], [M(1)]])
    assert rec == ([(2 << 4) | A.INS, (2 << 4) | A.EQ], [0], [2])
    assert A.expand(*rec)[:2] == [(None, "IB"), (None, "IB")] and A.cigar_string(rec[0]) == "2I2="


def test_clause_del_behind_ins_begin():
    # InsBegin, then a Del on node 0 in the same row, then Match on 1: the Del is the first step
    rec = _case(b"TC", [[IB, Dl(0)], [M(1)]])
    assert rec == ([(1 << 4) | A.INS, (1 << 4) | A.DEL, (1 << 4) | A.EQ], [0], [2])
    assert A.expand(*rec) == [(None, "IB"), (0, "D"), (1, "M")]


def test_clause_full_del_row():
    # n_max_gaps + 1 = 3 Dels in one row: one CIGAR run of 3; with the Match in front and behind one walk run of 5
    rec = _case(b"AA", [[M(0), Dl(1), Dl(2), Dl(3)], [M(4)]])
    assert rec == ([(1 << 4) | A.EQ, (3 << 4) | A.DEL, (1 << 4) | A.EQ], [0], [5])


def test_clause_end_on_a_del():
    rec = _case(b"AC", [[M(0)], [M(1), Dl(2)]])
    assert rec == ([(2 << 4) | A.EQ, (1 << 4) | A.DEL], [0], [3])
    assert A.expand(*rec)[-1] == (2, "D")


def test_clause_self_loop_twice_and_mismatch():
    # node 5 ('C') three times: three runs of length 1; its base against C, G, C: = X =
    rec = _case(b"CGC", [[M(5)], [M(5)], [M(5)]])
    assert rec == ([(1 << 4) | A.EQ, (1 << 4) | A.DIFF, (1 << 4) | A.EQ], [5, 5, 5], [1, 1, 1])


def test_clause_ascending_and_descending_ids():
    # the list names the nodes in another order: the walk goes by node id, not by slot
    lists = [[3, 2, 1, 0]] * 4
    up = _case(b"ACGT", [[M(3)], [M(2)], [M(1)], [M(0)]], lists)  # nodes 0 1 2 3
    down = _case(b"TGCA", [[M(0)], [M(1)], [M(2)], [M(3)]], lists)  # nodes 3 2 1 0
    assert up == ([(4 << 4) | A.EQ], [0], [4])
    assert down == ([(4 << 4) | A.EQ], [3, 2, 1, 0], [1, 1, 1, 1])


def test_clause_ins_on_a_node():
    # an I after a step sits on the last step's node, a Del included; Ins is no step and does not break a walk run
    rec = _case(b"ATCG", [[M(0)], [I(0)], [M(1), Dl(2)], [I(2)]])
    assert rec == ([(1 << 4) | A.EQ, (1 << 4) | A.INS, (1 << 4) | A.EQ, (1 << 4) | A.DEL, (1 << 4) | A.INS], [0], [3])
    assert A.expand(*rec) == [(0, "M"), (0, "I"), (1, "M"), (2, "D"), (2, "I")]


def test_clause_one_base_and_no_path():
    assert _case(b"G", [[M(2)]]) == ([(1 << 4) | A.EQ], [2], [1])
    assert _case(b"G", [[M(3)]]) == ([(1 << 4) | A.DIFF], [3], [1])
    assert _case(b"G", [[IB]], gaps=0) == ([(1 << 4) | A.INS], [], [])  # (no path of the model ends so; the record still reads)
    none = A.compress(_linear(), b"ACG", [FULL] * 3, _rows(4, [], [], []))
    assert none == ([], [], []) and A.expand(*none) == []
    A.check_invariants(*none, 3, [0, 0, 0, 0])
    assert A.compress(_linear(), b"", [], np.zeros((0, 4), dtype=np.uint32)) == ([], [], [])


def test_invariants_catch_a_wrong_record():
    good = ([(2 << 4) | A.EQ, (1 << 4) | A.DEL], [0], [3])
    A.check_invariants(*good, 2, [2, 0, 0, 1])
    for bad in (([(1 << 4) | A.EQ, (1 << 4) | A.EQ, (1 << 4) | A.DEL], [0], [3]),  # runs not maximal
                ([(2 << 4) | A.EQ, (1 << 4) | A.DEL], [0, 2], [2, 1]),             # walk runs not maximal
                ([(2 << 4) | A.EQ, (1 << 4) | A.DEL], [0], [2]),                   # a step short
                ([(3 << 4) | A.EQ, (1 << 4) | A.DEL], [0], [4])):                  # a base too many
        with pytest.raises(AssertionError):
            A.check_invariants(*bad, 2, [2, 0, 0, 1])


# ---------------------------------------------------------------- the host classes against the restatement
def _alignments(records, n_samples=0):
    op_off, run_off, ops, rn, rl = [0], [0], [], [], []
    for c, n, l in records:
        ops += c
        rn += n
        rl += l
        op_off.append(len(ops))
        run_off.append(len(rn))
    return D.Alignments.from_arrays(len(records) // max(n_samples, 1), n_samples, op_off, ops, run_off, rn, rl)


def _records():
    arrays, reads, lists = B.many_short_reads()
    recs = [A.compress(arrays, r, ls, B.best_path_ref(arrays, r, ls)[1]) for r, ls in zip(reads[:60], lists[:60])]
    recs[7] = recs[31] = ([], [], [])  # two reads without a path
    return recs


def test_model_alignments_against_expand():
    recs = _records()
    al = _alignments(recs)
    assert len(al) == 60 and any(not c for c, _, _ in recs) and any(c for c, _, _ in recs)
    for a, (c, n, l) in enumerate(recs):
        assert al.states(a) == A.expand(c, n, l)
        assert al.cigar(a) == [(w >> 4, w & 15) for w in c] and al.cigar_string(a) == A.cigar_string(c)
        assert al.walk(a) == list(zip(n, l)) and al.nodes(a) == [s[0] for s in A.expand(c, n, l) if s[1] in "MD"]
    al3 = _alignments(recs, n_samples=3)
    assert len(al3) == 60 and al3.n_reads == 20 and al3.index(4, 2) == 14 and al3.states(14) == A.expand(*recs[14])


@pytest.mark.parametrize("n_samples", [0, 3])
def test_formats_round_trip(n_samples):
    recs = _records()
    al = _alignments(recs, n_samples)
    R = al.n_reads
    names = [f"read{r}" for r in range(R)]
    for logp in (np.linspace(-50.0, -1.0, R), np.where(np.arange(60) % 7 == 0, -np.inf, -np.arange(60) / 3.0)):
        fh = io.StringIO()
        D.formats.write_alignments(fh, al, logp, names)
        text = fh.getvalue()
        assert len([ln for ln in text.splitlines() if not ln.startswith("#")]) == 60
        names2, logp2, al2 = D.formats.read_alignments(io.StringIO(text))
        assert names2 == names and al2.n_samples == n_samples and len(al2) == 60
        want = np.repeat(logp, max(n_samples, 1)) if logp.shape[0] == R and R != 60 else logp
        assert np.array_equal(logp2, want)
        for x, y in zip(al.arrays(), al2.arrays()):
            assert x.dtype == y.dtype and np.array_equal(x, y)
    fh = io.StringIO()
    D.formats.write_alignments(fh, al, np.zeros(R))  # without names: the read's index
    line = [ln for ln in fh.getvalue().splitlines() if not ln.startswith("#")][max(n_samples, 1)]
    assert line.split("\t")[:2] == ["1", "0"] and "GAF" not in fh.getvalue()
