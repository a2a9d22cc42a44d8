"""GPU: the best path of every read over its mapping lists (phmm_run_with_mapping_best_path,
PHMMModel.run_with_mapping_best_path): forward_with_mapping with every sum replaced by a maximum, and the walk back.

The reference has no Viterbi, so the feature checks itself (tests/best_path_ref.py, held on its own by
tests/test_best_path_ref_cpu.py): per read
  * out_logp equals best_path_ref, the recursion in Python, within the bar,
  * score_path accepts the GPU's rows as a legal path, re-scores them term by term from the model arrays to out_logp
    within the bar, and counts what out_counts counts,
  * out_logp <= the oracle's hinted forward ln P over the same lists + 1e-9 (the best path is one term of that sum).
The bar is 4 n_terms 2^-53 |ln P|: derived in best_path_ref.py, not tuned.  Lists come from generate_mappings on the
same handle, except the crafted widths (pad_lists) and the zero-error linear mock, where generate_mappings has no list to
give for a read of probability 0: there every position lists the whole graph."""
import ctypes as C

import numpy as np
import pytest

import dbgphmm_amd as D
import best_path_ref as B
from dbgphmm_amd import _ffi
from graph_cases import base_case, with_gaps, zoo_graph, zoo_model

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
