"""GPU: the best path of every read over its mapping lists (phmm_run_with_mapping_best_path,
PHMMModel.run_with_mapping_best_path): forward_with_mapping with every sum replaced by a maximum, and the walk back.

The reference has no Viterbi, so the feature checks itself (tests/best_path_ref.py, held on its own by
tests/test_best_path_ref_cpu.py, which also pins its tie rule to the header by brute force): per read
  * out_logp equals best_path_ref, the recursion in Python, as a double: the same additions in the same association,
  * out_path equals the reference's rows word for word (the header's tie rule leaves one path) and out_counts what
    score_path counts on them,
  * score_path accepts the GPU's rows as a legal path and re-scores them term by term from the model arrays to
    out_logp within the bar (that sum is taken in another order),
  * out_logp <= the oracle's hinted forward ln P over the same lists + 1e-9 (the best path is one term of that sum).
The bar is 4 n_terms 2^-53 |ln P|: derived in best_path_ref.py, not tuned.  Sections 7 to 13 feed what the header
promises beyond ordinary inputs: ties, odd lists, -inf parameters, both capacity classes and chunks on the same reads,
hundreds of reads, new numbers on one handle, relabelled graphs.  Lists come from generate_mappings on the
same handle, except the crafted widths (pad_lists) and the zero-error linear mock, where generate_mappings has no list to
give for a read of probability 0: there every position lists the whole graph."""
import ctypes as C

import numpy as np
import pytest

import dbgphmm_amd as D
import best_path_ref as B
from dbgphmm_amd import _ffi
from graph_cases import ORDERINGS, base_case, carry_mappings, relabelled_case, with_gaps, zoo_graph, zoo_model

pytestmark = pytest.mark.gpu
NONE = B.NONE
STATS_HINTED = 2


def _best_path(arrays, reads, lists=None):
    """-> (model, reads, mappings, (pos_off, nodes), logp, path, counts); lists = (pos_off, nodes) or None for the
    model's own generate_mappings"""
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    mp = gm.generate_mappings(rc, None, True)[0] if lists is None else D.Mappings.from_arrays(rc, lists[0], lists[1])
    lp, path, counts = gm.run_with_mapping_best_path(rc, mp)
    po, nd, _ = mp.arrays()
    assert path.shape == (rc.total_bases(), arrays.param.n_max_gaps + 2) and counts.shape == (len(reads), 4)
    return gm, rc, mp, (po, nd), lp, path, counts


def _parity(oracle, arrays, reads, rc, po, nd, lp, path, counts, what):
    """the three checks of the module docstring for every read -> the largest ln P(forward) - ln P(best path)"""
    om = oracle.Model(arrays)
    off = rc.offsets.astype(np.int64)
    gap, worst = 0.0, 0.0
    for j, r in enumerate(reads):
        lists = B.lists_of(po, nd, off[j], off[j + 1])
        want, n_terms = B.check_read(arrays, r, lists, float(lp[j]), path[off[j]:off[j + 1]], counts[j].tolist())
        total = om.forward_score_only(r, oracle.Mapping.from_lists(lists))
        assert lp[j] <= total + 1e-9, (what, j, lp[j], total)
        if want > -np.inf:
            gap = max(gap, total - lp[j])
            worst = max(worst, abs(lp[j] - want) / B.bar(n_terms, want))
    print(f"{what}: {len(reads)} reads, |out_logp - reference| at most {worst:.3f} of the bar, "
          f"largest ln P(forward) - ln P(best path) {gap:.3f}")
    return gap


def _states(mp, j, path):
    return D.path_states(mp, j, path)


# ------------------------------------------------------------------ 1. known answers on the linear mock
def test_linear_mock_zero_error(gpu_lib, oracle):
    a = B.linear(0.0)
    reads = [b"CGATC", b"CGATT"]
    n = sum(len(r) for r in reads)
    full = (np.arange(n + 1, dtype=np.uint64) * a.n_nodes, np.tile(np.arange(a.n_nodes, dtype=np.uint32), n))
    gm, rc, mp, (po, nd), lp, path, counts = _best_path(a, reads, full)
    total = oracle.Model(a).forward_score_only(reads[0], oracle.Mapping.from_lists(B.full_lists(a, reads[0])))
    assert abs(lp[0] - total) <= B.bar(16, total)  # one path only: the maximum is the sum
    assert _states(mp, 0, path) == [(v, "M") for v in range(3, 8)]
    assert counts[0].tolist() == [5, 0, 0, 0]
    assert lp[1] == -np.inf and np.all(path[5:] == NONE) and counts[1].tolist() == [0, 0, 0, 0]
    assert _states(mp, 1, path) == []
    _parity(oracle, a, reads, rc, po, nd, lp, path, counts, "linear mock, uniform(0)")


def test_linear_mock_with_errors(gpu_lib, oracle):
    a = B.linear(0.01)
    reads = [b"ATTCGTCGT",    # the reference's deletion read (freq.rs:499-514)
             b"ATTCGCATCGT",  # one inserted base
             b"ATTCGATGGT"]   # one substituted base
    gm, rc, mp, (po, nd), lp, path, counts = _best_path(a, reads)
    assert _states(mp, 0, path) == [(v, "M") for v in range(5)] + [(5, "D")] + [(v, "M") for v in range(6, 10)]
    assert path[4, 1] & 3 == 2 and np.all(np.delete(path[:9], 4, 0)[:, 1:] == NONE)  # the Del sits behind base 4
    assert counts[0].tolist() == [9, 0, 0, 1]
    assert _states(mp, 1, path) == [(v, "M") for v in range(5)] + [(4, "I")] + [(v, "M") for v in range(5, 10)]
    assert counts[1].tolist() == [10, 0, 1, 0]
    assert _states(mp, 2, path) == [(v, "M") for v in range(10)]
    assert counts[2].tolist() == [len(reads[2]) - 1, 1, 0, 0]
    _parity(oracle, a, reads, rc, po, nd, lp, path, counts, "linear mock, uniform(0.01)")


# ------------------------------------------------------------------ 2. parity on small graphs
@pytest.fixture(scope="module")
def dbg_run(gpu_lib):
    b = base_case("dbg")
    return (b,) + _best_path(b["arrays"], b["reads"])


def test_parity_dbg(oracle, dbg_run):
    b, gm, rc, mp, (po, nd), lp, path, counts = dbg_run
    _parity(oracle, b["arrays"], b["reads"], rc, po, nd, lp, path, counts, "dbg")


@pytest.mark.parametrize("graph", ["zoo", "zoo_lean"])
def test_parity_zoo(gpu_lib, oracle, graph):
    """the zoo graph with its self-loop, parallel edge and hub of degree 7 (zoo), and without the hub (zoo_lean)"""
    b = base_case(graph)
    gm, rc, mp, (po, nd), lp, path, counts = _best_path(b["arrays"], b["reads"])
    _parity(oracle, b["arrays"], b["reads"], rc, po, nd, lp, path, counts, graph)


@pytest.mark.parametrize("which", range(6))
def test_parity_fuzz(gpu_lib, oracle, which):
    c = B.fuzz_cases()[which]
    gm, rc, mp, (po, nd), lp, path, counts = _best_path(c["arrays"], c["reads"])
    _parity(oracle, c["arrays"], c["reads"], rc, po, nd, lp, path, counts, c["tag"])


# ------------------------------------------------------------------ 3. Del levels
@pytest.mark.parametrize("gaps", [0, 4, 6])
def test_del_levels(gpu_lib, oracle, gaps):
    arrays, read = B.two_deletions()
    a = with_gaps(arrays, gaps)
    gm, rc, mp, (po, nd), lp, path, counts = _best_path(a, [read])
    assert path.shape[1] == gaps + 2 == (2, 6, 8)[(0, 4, 6).index(gaps)]
    _parity(oracle, a, [read], rc, po, nd, lp, path, counts, f"two adjacent deletions, n_max_gaps = {gaps}")
    dels = (path[:, 1:] != NONE).sum(axis=1)
    if gaps == 0:
        assert dels.max() <= 1  # no row holds more than one Del
    else:
        assert dels.max() == 2 and counts[0].tolist() == [len(read), 0, 0, 2]


# ------------------------------------------------------------------ 4. list widths: both capacity classes and their edges
def _gpu_lists(arrays, reads):
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    po, nd, _ = gm.generate_mappings(rc, None, True)[0].arrays()
    return po, nd


@pytest.mark.parametrize("width", B.WIDTHS)
def test_list_widths(gpu_lib, oracle, width):
    arrays, reads = B.width_reads(width)
    po0, nd0 = _gpu_lists(arrays, reads)
    ppo, pnd = B.pad_lists(po0, nd0, reads, arrays.n_nodes, width)
    assert int(np.diff(ppo.astype(np.int64)).max()) == width  # (on the CPU: the longest list of the case)
    gm, rc, mp, (po, nd), lp, path, counts = _best_path(arrays, reads, (ppo, pnd))
    assert np.all(np.isfinite(lp))
    _parity(oracle, arrays, reads, rc, po, nd, lp, path, counts, f"lists padded to {width}")
    ms, launches, cells = _ffi.last_call_stats(STATS_HINTED)
    assert cells == int(ppo[-1]) and launches == 2  # one capacity class and the walk back


class _Prefilled:
    """sentinel-filled outputs of one call"""

    def __init__(self, rc, stride=8):
        self.lp = np.full(max(len(rc), 1), 7.5)
        self.path = np.full((max(rc.total_bases(), 1), stride), 77, dtype=np.uint32)
        self.counts = np.full((max(len(rc), 1), 4), 77, dtype=np.uint32)

    def call(self, gm, rc, mp):
        P = lambda a: a.ctypes.data_as(C.c_void_p)
        _ffi.check(_ffi.lib().phmm_run_with_mapping_best_path(gm._h, rc._h, mp._h, P(self.lp), P(self.path), P(self.counts)))

    def untouched(self):
        return bool(np.all(self.lp == 7.5) and np.all(self.path == 77) and np.all(self.counts == 77))


def _status(f):
    try:
        f()
    except _ffi.PhmmError as e:
        return e.code
    return _ffi.PHMM_OK


def test_width_401_is_refused(gpu_lib):
    arrays, reads = B.width_reads(400)
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    n = rc.total_bases()
    out = _Prefilled(rc)

    def call():  # (a list of 401 is refused where the lists are handed over)
        over = D.Mappings.from_arrays(rc, np.arange(n + 1, dtype=np.uint64) * 401, np.tile(np.arange(401, dtype=np.uint32), n))
        out.call(gm, rc, over)
    assert _status(call) == _ffi.PHMM_ECAPACITY and out.untouched()


# ------------------------------------------------------------------ 5. one long read
def test_long_read(gpu_lib, oracle):
    arrays, read = B.long_read()
    gm, rc, mp, (po, nd), lp, path, counts = _best_path(arrays, [read])
    assert len(read) == 3000 and np.isfinite(lp[0])
    _parity(oracle, arrays, [read], rc, po, nd, lp, path, counts, "one read of 3000 bases")


# ------------------------------------------------------------------ 6. plumbing
class _DeviceArray:
    """bytes in device memory (the HIP runtime the library is linked against)"""

    def __init__(self, nbytes, fill):
        self.hip, self.nbytes = C.CDLL("libamdhip64.so"), nbytes
        self.p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.p), C.c_size_t(max(nbytes, 1))) == 0
        assert self.hip.hipMemset(self.p, C.c_int(fill), C.c_size_t(max(nbytes, 1))) == 0

    def numpy(self, dtype):
        out = np.empty(self.nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        assert self.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), self.p, C.c_size_t(self.nbytes), 2) == 0
        return out

    def __del__(self):
        self.hip.hipFree(self.p)


def test_output_forms(gpu_lib, dbg_run):
    """device-pointer outputs equal host-pointer outputs bit for bit; out_path = NULL leaves the other two unchanged;
    every output may be NULL; a call without reads writes nothing"""
    b, gm, rc, mp, _, lp, path, counts = dbg_run
    L, R, n = _ffi.lib(), len(rc), rc.total_bases()
    dl, dp, dc = _DeviceArray(8 * R, 0), _DeviceArray(4 * path.shape[1] * n, 0), _DeviceArray(16 * R, 0)
    _ffi.check(L.phmm_run_with_mapping_best_path(gm._h, rc._h, mp._h, dl.p, dp.p, dc.p))
    assert np.array_equal(dl.numpy(np.float64), lp)
    assert np.array_equal(dp.numpy(np.uint32).reshape(path.shape), path)
    assert np.array_equal(dc.numpy(np.uint32).reshape(counts.shape), counts)
    lp2, none, counts2 = gm.run_with_mapping_best_path(rc, mp, want_path=False)
    assert none is None and np.array_equal(lp2, lp) and np.array_equal(counts2, counts)
    _ffi.check(L.phmm_run_with_mapping_best_path(gm._h, rc._h, mp._h, None, None, None))
    rc0 = D.ReadCollection([])
    mp0 = D.Mappings.from_arrays(rc0, np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint32))
    out = _Prefilled(rc0)
    out.call(gm, rc0, mp0)
    assert out.untouched()


def test_a_read_alone_and_a_second_call(gpu_lib, dbg_run):
    """a read scored alone gives the bits it gets inside the set; a second identical call returns the same bits and
    allocates nothing (phmm_reads_create takes no empty read, so the -inf of an empty read cannot be asked for here)"""
    b, gm, rc, mp, (po, nd), lp, path, counts = dbg_run
    lp2, path2, counts2 = gm.run_with_mapping_best_path(rc, mp)
    ws = gpu_lib.phmm_workspace_bytes()
    lp3, path3, counts3 = gm.run_with_mapping_best_path(rc, mp)
    assert gpu_lib.phmm_workspace_bytes() == ws
    for x, y, z in ((lp, lp2, lp3), (path, path2, path3), (counts, counts2, counts3)):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    off = rc.offsets.astype(np.int64)
    for j in (0, 5, len(rc) - 1):
        rc1 = D.ReadCollection([b["reads"][j]])
        e0, e1 = int(po[off[j]]), int(po[off[j + 1]])
        mp1 = D.Mappings.from_arrays(rc1, po[off[j]:off[j + 1] + 1] - po[off[j]], nd[e0:e1])
        lp1, path1, counts1 = gm.run_with_mapping_best_path(rc1, mp1)
        assert lp1[0] == lp[j] and np.array_equal(path1, path[off[j]:off[j + 1]]) and np.array_equal(counts1[0], counts[j])


def test_workspace_limit_runs_the_reads_in_chunks(gpu_lib, dbg_run):
    b, gm, rc, mp, (po, nd), lp, path, counts = dbg_run
    off = rc.offsets.astype(np.int64)
    per_read = [16 * (int(po[off[j + 1]]) - int(po[off[j]])) + 4 * path.shape[1] * int(off[j + 1] - off[j]) for j in range(len(rc))]
    limit = 2 * max(per_read) + (64 << 10)  # records and staged rows of two reads or more, beside the call's fixed arrays
    assert 2 * max(per_read) < sum(per_read) / 2  # (at least two chunks)
    _ffi.check(gpu_lib.phmm_set_workspace_limit(limit))
    try:
        lp2, path2, counts2 = gm.run_with_mapping_best_path(rc, mp)
        ms, launches, cells = _ffi.last_call_stats(STATS_HINTED)
    finally:
        _ffi.check(gpu_lib.phmm_set_workspace_limit(0))
    assert launches >= 4 and cells == int(po[-1])  # at least two chunks: a forward class and a walk back each
    assert np.array_equal(lp2, lp) and np.array_equal(path2, path) and np.array_equal(counts2, counts)
    lp3, _, counts3 = gm.run_with_mapping_best_path(rc, mp, want_path=False)
    assert _ffi.last_call_stats(STATS_HINTED)[1] == 2 and np.array_equal(lp3, lp) and np.array_equal(counts3, counts)


def test_refusals(gpu_lib, dbg_run):
    """those of phmm_run_with_mapping_states, each with sentinel-filled outputs unchanged"""
    b, gm, rc, mp, (po, nd), lp, path, counts = dbg_run
    L = _ffi.lib()
    out = _Prefilled(rc)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    for h in ((None, rc._h, mp._h), (gm._h, None, mp._h), (gm._h, rc._h, None)):
        assert L.phmm_run_with_mapping_best_path(*h, P(out.lp), P(out.path), P(out.counts)) == _ffi.PHMM_EINVAL
    # mappings of another read set
    rc2 = D.ReadCollection(b["reads"][:2])
    assert _status(lambda: out.call(gm, rc2, mp)) == _ffi.PHMM_EINVAL
    # the degree limit: a hub of 9 arms
    sg = zoo_graph(arms=9)
    hub = D.PHMMModel(zoo_model(sg))
    reads = [b"ACGTACGT"]
    rch = D.ReadCollection(reads)
    mph = D.Mappings.from_arrays(rch, np.arange(9, dtype=np.uint64) * 3, np.tile(np.array([59, 60, 61], dtype=np.uint32), 8))
    out2 = _Prefilled(rch)
    got = _status(lambda: out2.call(hub, rch, mph))
    states = _status(lambda: hub.run_with_mapping_states(rch, mph))
    assert got == states == _ffi.PHMM_EINVAL
    assert out.untouched() and out2.untouched()


# ------------------------------------------------------------------ 7. ties
def _call(gm, reads, per_read_lists):
    """one call on an existing handle with lists[read][pos] -> (rc, mp, (pos_off, nodes), logp, path, counts)"""
    rc = D.ReadCollection(reads)
    po, nd = B.csr(per_read_lists)
    mp = D.Mappings.from_arrays(rc, po, nd)
    lp, path, counts = gm.run_with_mapping_best_path(rc, mp)
    assert path.shape == (rc.total_bases(), gm.param.n_max_gaps + 2) and counts.shape == (len(reads), 4)
    return rc, mp, (po, nd), lp, path, counts


def _same_bits(x, y):
    return all(np.array_equal(a, b) for a, b in zip(x, y))


def _path_nodes(per_read_lists, reads, path):
    """per read the node of every node state of its path, in order"""
    out, g = [], 0
    for lists, r in zip(per_read_lists, reads):
        out.append([lists[i][c >> 2] for i in range(len(r)) for c in path[g + i].tolist() if c not in (NONE, B.INS_BEGIN)])
        g += len(r)
    return out


def test_ties_bubble(gpu_lib, oracle):
    arrays, read, orders = B.bubble_case()
    gm = D.PHMMModel(arrays)
    values = set()
    for name, (order, nodes) in orders.items():
        lists = [[order] * len(read)]
        rc, mp, (po, nd), lp, path, counts = _call(gm, [read], lists)
        _parity(oracle, arrays, [read], rc, po, nd, lp, path, counts, f"bubble, list order {name}")
        assert _states(mp, 0, path) == [(v, "M") for v in nodes]
        values.add(float(lp[0]))
    assert len(values) == 1


@pytest.mark.parametrize("graph", ["zoo", "dbg"])
def test_ties_integer_logs(gpu_lib, oracle, graph):
    """every log an integer: equal path values are equal doubles and the rank decides; the same reads with every list
    reversed give the same values bit for bit and, where there was a tie between two nodes, another path"""
    c = B.int_case(graph)
    gm = D.PHMMModel(c["arrays"])
    rev = B.reversed_lists(c["lists"])
    rc, mp, (po, nd), lp, path, counts = _call(gm, c["reads"], c["lists"])
    _parity(oracle, c["arrays"], c["reads"], rc, po, nd, lp, path, counts, f"integer-log {graph}")
    rc2, mp2, (po2, nd2), lp2, path2, counts2 = _call(gm, c["reads"], rev)
    _parity(oracle, c["arrays"], c["reads"], rc2, po2, nd2, lp2, path2, counts2, f"integer-log {graph}, lists reversed")
    assert np.array_equal(lp, lp2) and np.all(np.isfinite(lp))
    a, b = _path_nodes(c["lists"], c["reads"], path), _path_nodes(rev, c["reads"], path2)
    differ = sum(x != y for x, y in zip(a, b))
    print(f"integer-log {graph}: {differ} of {len(a)} paths differ between the two list orders")
    assert differ >= 1


# ------------------------------------------------------------------ 8. odd lists and -inf parameters
@pytest.mark.parametrize("flavour", ["ord", "int"])
def test_odd_lists(gpu_lib, oracle, flavour):
    """duplicated entries, empty lists, unsorted lists, reads of one base, a node that leaves and comes back, each
    parameter at -inf, init on one node, and the forced path forms (tests/best_path_ref.py::odd_cases)"""
    n = finite = 0
    for g in B.odd_cases(flavour):
        rc, mp, (po, nd), lp, path, counts = _call(D.PHMMModel(g["arrays"]), g["reads"], g["lists"])
        _parity(oracle, g["arrays"], g["reads"], rc, po, nd, lp, path, counts, g["tag"])
        n, finite = n + len(lp), finite + int(np.isfinite(lp).sum())
        if g["tag"].endswith("forms, p_mismatch = -inf, init on node 2"):  # path_states on InsBegin rows
            j = g["reads"].index(b"AATT")
            assert _states(mp, j, path) == [(None, "IB"), (None, "IB"), (2, "D"), (3, "M"), (4, "M")]
            assert counts[j].tolist() == [2, 0, 2, 1]
    assert 2 * finite >= n and finite < n


# ------------------------------------------------------------------ 9. the same bits in both capacity classes
def _padding_sets(which):
    """-> [(tag, arrays with isolated nodes, first isolated node, reads, lists[read][pos])]"""
    if which == "integer-log zoo":
        c = B.int_case("zoo")
        return [(which, c["arrays"], c["n_real"], c["reads"], c["lists"])]
    return [(g["tag"], B.with_isolated(g["arrays"]), g["arrays"].n_nodes, g["reads"], g["lists"]) for g in B.odd_cases(which)]


@pytest.mark.parametrize("which", ["integer-log zoo", "ord", "int"])
def test_unreachable_padding_same_bits(gpu_lib, which):
    """lists of the <= 64 class, then the same lists padded with isolated nodes (-inf in every state) behind their
    entries to 65, 129 and 400 and in front of them to 400: the 400 class must return the bits of the 64 class, with the
    slots shifted where the padding stands in front (chosen slots then pass 255 and reach 399).  Every odd-list group
    and the integer-log zoo reads."""
    top, past_255 = 0, 0
    for n_set, (tag, arrays, first_pad, reads, lists) in enumerate(_padding_sets(which)):
        gm = D.PHMMModel(arrays)
        rc, mp, (po, nd), lp, path, counts = _call(gm, reads, lists)
        assert _ffi.last_call_stats(STATS_HINTED)[1] == 2
        off = rc.offsets.astype(np.int64)
        for j, (r, ls) in enumerate(zip(reads, lists)):
            B.check_read(arrays, r, ls, float(lp[j]), path[off[j]:off[j + 1]], counts[j].tolist())
        for width in (65, 129, 400):
            padded = [B.pad_unreachable(ls, first_pad, width, front=False) for ls in lists]
            _, _, _, lp2, path2, counts2 = _call(gm, reads, padded)
            assert _ffi.last_call_stats(STATS_HINTED)[1] == 2
            assert _same_bits((lp, path, counts), (lp2, path2, counts2)), (tag, width)
        padded = [B.pad_unreachable(ls, first_pad, 400, front=True) for ls in lists]
        _, _, (po3, nd3), lp3, path3, counts3 = _call(gm, reads, padded)
        want = np.concatenate([B.shift_slots(path[o:o + len(r)], ls, 400) for o, r, ls in zip(off, reads, lists)])
        assert np.array_equal(lp3, lp) and np.array_equal(counts3, counts) and np.array_equal(path3, want), tag
        slots = path3[(path3 != NONE) & (path3 != B.INS_BEGIN)] >> 2
        if slots.size:
            top, past_255 = max(top, int(slots.max())), past_255 + int((slots > 255).sum())
        if n_set == 0:  # (and against the reference over the wide lists themselves, for two reads)
            for j in range(2):
                B.check_read(arrays, reads[j], B.lists_of(po3, nd3, off[j], off[j + 1]), float(lp3[j]), path3[off[j]:off[j + 1]],
                             counts3[j].tolist())
    assert top == 399 and past_255 > 0


# ------------------------------------------------------------------ 10. both classes in one call, and chunks
def test_both_classes_in_one_call(gpu_lib, oracle):
    c = B.int_case("zoo")
    arrays, reads = c["arrays"], c["reads"]
    lists = [ls if j % 2 == 0 else B.pad_unreachable(ls, c["n_real"], 129, front=False) for j, ls in enumerate(c["lists"])]
    gm = D.PHMMModel(arrays)
    rc, mp, (po, nd), lp, path, counts = _call(gm, reads, lists)
    assert _ffi.last_call_stats(STATS_HINTED)[1] == 3  # the <= 64 class, the 400 class (its id list reuses the first's), the walk
    _parity(oracle, arrays, reads, rc, po, nd, lp, path, counts, "narrow and wide reads interleaved")
    off = rc.offsets.astype(np.int64)
    for j, (r, ls) in enumerate(zip(reads, lists)):
        _, _, _, lp1, path1, counts1 = _call(gm, [r], [ls])
        assert lp1[0] == lp[j] and np.array_equal(path1, path[off[j]:off[j + 1]]) and np.array_equal(counts1[0], counts[j]), j
    per_read = [16 * sum(len(x) for x in ls) + 4 * path.shape[1] * len(r) for r, ls in zip(reads, lists)]
    limit = 2 * max(per_read) + (64 << 10)  # (sized as test_workspace_limit_runs_the_reads_in_chunks)
    assert sum(per_read) > 2 * limit  # at least three chunks: no chunk holds more than the limit
    _ffi.check(gpu_lib.phmm_set_workspace_limit(limit))
    try:
        lp2, path2, counts2 = gm.run_with_mapping_best_path(rc, mp)
        launches = _ffi.last_call_stats(STATS_HINTED)[1]
    finally:
        _ffi.check(gpu_lib.phmm_set_workspace_limit(0))
    assert launches >= 6
    assert _same_bits((lp, path, counts), (lp2, path2, counts2))


# ------------------------------------------------------------------ 11. many short reads
def _chunks(per_read, budget):
    """the chunks of consecutive reads as best_path.hip cuts them -> [(r0, r1)]"""
    out, r0 = [], 0
    while r0 < len(per_read):
        r1, used = r0, 0
        while r1 < len(per_read) and (r1 == r0 or used + per_read[r1] <= budget):
            used += per_read[r1]
            r1 += 1
        out.append((r0, r1))
        r0 = r1
    return out


def test_many_short_reads(gpu_lib, oracle):
    """320 reads: five blocks of the walk back and two of the entry offsets; then in chunks of more than 64 reads, so
    that a walk back of several blocks starts at a read other than 0"""
    arrays, reads, lists = B.many_short_reads()
    gm = D.PHMMModel(arrays)
    rc, mp, (po, nd), lp, path, counts = _call(gm, reads, lists)
    assert len(reads) > 256 and _ffi.last_call_stats(STATS_HINTED)[1] == 2
    _parity(oracle, arrays, reads, rc, po, nd, lp, path, counts, f"{len(reads)} short reads")
    R = len(reads)
    per_read = [16 * sum(len(x) for x in ls) + 4 * path.shape[1] * len(r) for r, ls in zip(reads, lists)]
    fixed = 0
    for nbytes in (8 * R, 8 * (R + 1), 4 * R, 4 * R, 4 * R, 16 * R):  # the call's control arrays, each at a multiple of 256
        fixed = (fixed + 255) // 256 * 256 + nbytes
    fixed += 8 * (arrays.n_nodes + arrays.n_edges)
    budget = sum(per_read) * 2 // 5
    chunks = _chunks(per_read, budget)
    assert len(chunks) >= 2 and any(r0 > 0 and r1 - r0 > 64 for r0, r1 in chunks), chunks
    _ffi.check(gpu_lib.phmm_set_workspace_limit(fixed + budget))
    try:
        lp2, path2, counts2 = gm.run_with_mapping_best_path(rc, mp)
        launches = _ffi.last_call_stats(STATS_HINTED)[1]
    finally:
        _ffi.check(gpu_lib.phmm_set_workspace_limit(0))
    assert launches == 2 * len(chunks), (launches, chunks)  # (the library cut the reads where this test expects it)
    assert _same_bits((lp, path, counts), (lp2, path2, counts2))


# ------------------------------------------------------------------ 12. the same handle with new numbers
def test_same_handle_new_numbers(gpu_lib, oracle):
    """after phmm_model_set_probs and phmm_model_set_params the call follows the handle's current numbers: the bits of
    a fresh model, and the row stride of the new n_max_gaps"""
    g = [g for g in B.odd_cases("ord") if g["tag"].endswith("list oddities, n_max_gaps = 2")][0]
    a1, reads, lists = g["arrays"], g["reads"], g["lists"]
    a3 = B.odd_arrays("int", 0)  # other init, trans and parameters on the same graph
    a2 = D.PHMMArrays(a1.param, a1.emission, a3.init_logp, a1.edge_src, a1.edge_dst, a3.trans_logp)
    gm = D.PHMMModel(a1)
    first = _call(gm, reads, lists)
    gm.set_probs(a2.init_logp, a2.trans_logp)
    rc, mp, (po, nd), lp, path, counts = _call(gm, reads, lists)
    _parity(oracle, a2, reads, rc, po, nd, lp, path, counts, "after set_probs")
    assert _same_bits((lp, path, counts), _call(D.PHMMModel(a2), reads, lists)[3:])
    assert not np.array_equal(lp, first[3])
    cp = a3.param.to_c()
    _ffi.check(_ffi.lib().phmm_model_set_params(gm._h, C.byref(cp)))
    gm.param = a3.param  # (PHMMModel sizes the rows by its param)
    rc, mp, (po, nd), lp, path, counts = _call(gm, reads, lists)
    assert path.shape[1] == 2
    _parity(oracle, a3, reads, rc, po, nd, lp, path, counts, "after set_params, n_max_gaps 2 -> 0")
    assert _same_bits((lp, path, counts), _call(D.PHMMModel(a3), reads, lists)[3:])


# ------------------------------------------------------------------ 13. relabelling
@pytest.fixture(scope="module")
def zoo_run(gpu_lib):
    b = base_case("zoo")
    return (b,) + _best_path(b["arrays"], b["reads"])


@pytest.mark.parametrize("ordering", ORDERINGS)
@pytest.mark.parametrize("graph", ["dbg", "zoo"])
def test_relabelling(gpu_lib, dbg_run, zoo_run, graph, ordering):
    """other node ids and another edge order, the lists carried onto the new ids in the same slot order: ranks go by
    slot and an edge permutation only reorders candidates of equal rank, so every output keeps its bits"""
    b, gm, rc, mp, (po, nd), lp, path, counts = dbg_run if graph == "dbg" else zoo_run
    case = relabelled_case(graph, ordering)
    po2, nd2, _ = carry_mappings((po, nd, None), case["node_perm"])
    _, rc2, _, _, lp2, path2, counts2 = _best_path(case["arrays"], b["reads"], (po2, nd2))
    assert _same_bits((lp, path, counts), (lp2, path2, counts2))
    off = rc2.offsets.astype(np.int64)
    for j in (0, 7, 11):  # (and against the reference on the new labels)
        B.check_read(case["arrays"], b["reads"][j], B.lists_of(po2, nd2, off[j], off[j + 1]), float(lp2[j]),
                     path2[off[j]:off[j + 1]], counts2[j].tolist())


# ------------------------------------------------------------------ 14. one more refusal
def test_node_out_of_range_is_refused(gpu_lib, dbg_run):
    """a list that names a node >= n_nodes: refused on the host (check_mapping_nodes) before anything is launched"""
    b, gm, rc, mp, (po, nd), lp, path, counts = dbg_run
    bad = nd.copy()
    bad[len(bad) // 2] = b["arrays"].n_nodes
    out = _Prefilled(rc)
    assert _status(lambda: out.call(gm, rc, D.Mappings.from_arrays(rc, po, bad))) == _ffi.PHMM_EINVAL and out.untouched()
