"""GPU: per-read transition usage over mapping lists (phmm_run_with_mapping_read_edges,
PHMMModel.run_with_mapping_read_edges, include/phmm_amd_edges.h): PHMMOutput::to_edge_and_init_freqs() (freq.rs:276-298)
of every read on its lists, as a sparse read-by-key matrix reduced on the device from the records of the edge list pass.

The bars.
  1. Per read against the oracle's run_with_mapping(read, its lists).to_edge_and_init_freqs(): TOL_FREQ = 1e-9 absolute,
     the bar tests/test_gpu_hinted_edges.py holds the summed call to per read.  A key absent from the row counts as 0.
  2. Against the summed call (run_with_mapping_edge_freqs): ln P bit for bit, the totals within 1e-9 * R.
  3. On the raw bits: the totals are the column sums of the exported rows by the header's order rule; a read's row does
     not depend on the other reads; two calls and the two output forms agree.
  4. A key map's row against the default-key row folded through the map in numpy: (n + 4) * 2^-52 relative, n an upper
     bound on the terms behind the entry.  Both are sums of the same non-negative terms (the read's records on the
     edges of the key) in two orders, each within (n - 1) * 2^-53 relative of the exact sum, so they differ by at most
     (n - 1) * 2^-52; a default-key entry of a read of L bases has at most 6 (L + 1) records (six transition kinds at
     L + 1 merged indices), so n = 6 (L + 1) m for m entries folded.
The reduction does not chunk (the header: it refuses with PHMM_ECAPACITY instead), so there is no chunked case."""
import ctypes as C
import gc
import json
import os

import numpy as np
import pytest

import caller_cases as cc
import dbgphmm_amd as D
from dbgphmm_amd import _ffi, _ffi_edges
from helpers import small_dbg_model, subset_csr
from repeat_cases import dataset

pytestmark = pytest.mark.gpu
KAT = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "kat_hmmv2.json")))
TOL_FREQ = 1e-9
EPS = 2.0 ** -52
STATS_REDUCE, STATS_WIDE = 2, 4
NO_KEY = D.PHMM_NO_KEY
KNOBS = ("PHMM_WIDE_HINTED", "PHMM_NO_WIDE_HINTED", "PHMM_WIDE_STATES_BWD", "PHMM_WIDE_EDGE_BWD", "PHMM_NO_WIDE_LIST_BWD",
         "PHMM_WIDE_BWD_T")
BLOCK = {"PHMM_WIDE_HINTED": "1", "PHMM_WIDE_EDGE_BWD": "1"}
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731


class _knobs:
    """exactly these knobs for the calls inside the block (knobs are read when a call takes the device)"""

    def __init__(self, setting):
        self.setting = dict(setting)

    def __enter__(self):
        self.before = {k: os.environ.get(k) for k in KNOBS}
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(self.setting)

    def __exit__(self, *a):
        for k, v in self.before.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class _Run:
    """one run_with_mapping_read_edges call, its rows on the host, and index 2 of its statistics"""

    def __init__(self, gm, rc, mp, **kw):
        self.lf, self.u = gm.run_with_mapping_read_edges(rc, mp, **kw)
        self.stats = _ffi.last_call_stats(STATS_REDUCE)
        self.row_off, self.keys, self.usage = self.u.arrays()
        self.totals, self.end_terms = self.u.totals, self.u.end_terms

    def same_bits(self, other):
        return all(cc.same_bits(np.asarray(a), np.asarray(b)) for a, b in
                   ((self.lf, other.lf), (self.row_off, other.row_off), (self.keys, other.keys), (self.usage, other.usage),
                    (self.totals, other.totals), (self.end_terms, other.end_terms)))


def _all_nodes(rc, n_nodes):
    """every node listed at every position"""
    T = int(rc.offsets[-1])
    return D.Mappings.from_arrays(rc, np.arange(T + 1, dtype=np.uint64) * n_nodes, np.tile(np.arange(n_nodes), T))


def rule_two(terms):
    """the header's second rule: 64 strided partial sums from 0, then the xor butterfly 32 .. 1 -> p_0"""
    p = [0.0] * 64
    for i, t in enumerate(terms):
        p[i % 64] += t
    for d in (32, 16, 8, 4, 2, 1):
        p = [p[l] + p[l ^ d] for l in range(64)]
    return p[0]


def _well_formed(run, n_reads, n_keys):
    assert run.row_off.shape == (n_reads + 1,) and run.row_off[0] == 0 and int(run.row_off[-1]) == run.keys.size
    assert np.all(np.diff(run.row_off.astype(np.int64)) >= 0)
    for r in range(n_reads):
        k = run.u.row(r)[0].astype(np.int64)
        assert np.all(np.diff(k) > 0) and (k.size == 0 or k[-1] < n_keys)  # distinct, ascending
    assert np.all(np.isfinite(run.usage)) and np.all(run.usage > 0.0)  # a key of zero terms is not in the row


def _check_oracle_per_read(oracle, arrays, reads, rc, mp, run, what):
    """bar 1 -> the largest end term init_v (A_r + T_r e_v) met"""
    om = oracle.Model(arrays)
    off = rc.offsets.astype(np.int64)
    arr = mp.arrays()
    init = np.exp(arrays.init_logp)
    worst_e = worst_i = worst_l = big_end = 0.0
    for i, r in enumerate(reads):
        o = om.run_with_mapping(r, oracle.Mapping(*subset_csr(off, arr, [i])))
        oef, oinf = o.to_edge_and_init_freqs()
        ef, inf = run.u.edge_freqs(i), run.u.init_freqs(i, arrays, r[-1])
        worst_l = max(worst_l, abs(run.lf[i] - o.to_full_prob_forward()))
        worst_e = max(worst_e, float(np.max(np.abs(ef - oef))) if ef.size else 0.0)
        worst_i = max(worst_i, float(np.max(np.abs(inf - oinf))))
        big_end = max(big_end, float(np.max(inf - run.u.key_freqs(i)[arrays.n_edges:])))
    print(f"{what}: per read against the oracle max |d| ln P {worst_l:.3e}, edges {worst_e:.3e}, init {worst_i:.3e}; "
          f"largest end term {big_end:.3e}")
    assert worst_l < TOL_FREQ and worst_e < TOL_FREQ and worst_i < TOL_FREQ
    assert np.all(init >= 0.0)
    return big_end


def _totals_by_the_rule(run):
    cols = [[] for _ in range(run.totals.shape[0])]
    for k, x in zip(run.keys.tolist(), run.usage.tolist()):
        cols[k].append(x)  # (CSR order is read order)
    return np.array([rule_two(c) for c in cols])


# ------------------------------------------------------------------ 1. the reference's own assertions, per read
def test_linear_cgatc_at_zero_error(gpu_lib):
    """Fails without the feature: the call does not exist.  freq.rs:517-609 with every node listed."""
    arrays = D.mock_linear().to_phmm(D.PHMMParams.zero_error())
    gm, rc = D.PHMMModel(arrays), D.ReadCollection([b"CGATC"])
    with _knobs({}), np.errstate(divide="ignore"):
        run = _Run(gm, rc, _all_nodes(rc, arrays.n_nodes))
    _well_formed(run, 1, arrays.n_edges + arrays.n_nodes)
    ef = run.u.edge_freqs(0)
    assert ef.shape == (arrays.n_edges,)
    assert np.all(ef[3:7] > 0.9999) and np.all(ef[[0, 1, 2, 7, 8]] < 1e-4)
    assert run.stats[2] > 0 and run.stats[1] > 0  # cells = records reduced


def test_crossing_edge_37(gpu_lib):
    """seq_graph.rs:494-500: edge 37 is used (0.99992) without edge copy numbers"""
    rb = KAT["crossing"]["read"].encode()
    arrays = D.mock_crossing(False).to_phmm(D.PHMMParams.default())
    gm, rc = D.PHMMModel(arrays), D.ReadCollection([rb])
    with _knobs({}):
        run = _Run(gm, rc, _all_nodes(rc, arrays.n_nodes))
        _, sef, _ = gm.run_with_mapping_edge_freqs(rc, _all_nodes(rc, arrays.n_nodes))
    ef = run.u.edge_freqs(0)
    assert abs(ef[37] - 0.99992) < 1e-5
    assert np.max(np.abs(ef - sef)) < TOL_FREQ  # (one read: the summed call is its row)


# ------------------------------------------------------------------ 2. generated lists against the oracle, per read
def _fixture_reads(n_reads):
    arrays, sg = small_dbg_model(300, 12, 0.01, seed=5)
    reads = D.sample_reads(arrays, 10 ** 9, 60, seed=n_reads, max_reads=n_reads)
    return arrays, sg, [r[: max(1, len(r) - (j * 7) % 31)] for j, r in enumerate(reads)]


@pytest.fixture(scope="module")
def fix70(gpu_lib):
    arrays, sg, reads = _fixture_reads(70)
    assert len(reads) == 70
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    with _knobs({}):
        mp, _ = gm.generate_mappings(rc, None, True)
        run = _Run(gm, rc, mp)
    return arrays, sg, reads, gm, rc, mp, run


@pytest.mark.parametrize("n_reads", [1, 5, 70])
def test_generated_lists_match_oracle_per_read(gpu_lib, oracle, fix70, n_reads):
    if n_reads == 70:
        arrays, _, reads, gm, rc, mp, run = fix70
    else:
        arrays, _, reads = _fixture_reads(n_reads)
        gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
        with _knobs({}):
            mp, _ = gm.generate_mappings(rc, None, True)
            run = _Run(gm, rc, mp)
    E, N = arrays.n_edges, arrays.n_nodes
    _well_formed(run, n_reads, E + N)
    assert len(run.u) == n_reads and run.u.n_keys == E + N and run.totals.shape == (E + N,) and run.end_terms.shape == (n_reads, 2)
    _check_oracle_per_read(oracle, arrays, reads, rc, mp, run, f"generated lists, {n_reads} reads")
    assert run.stats[1] > 0 and run.stats[2] >= run.keys.size  # a row entry sums at least one record
    # reads_of is the transpose of row
    uk = np.unique(run.keys)
    for key in uk[:: max(1, uk.size // 25)].tolist():
        rd, us = run.u.reads_of(key)
        assert rd.tolist() == [r for r in range(n_reads) if key in run.u.row(r)[0]]
        for r, x in zip(rd.tolist(), us.tolist()):
            keys, usage = run.u.row(r)
            assert usage[np.searchsorted(keys, key)] == x


def test_lists_of_the_400_slot_class(gpu_lib, oracle):
    """u20n200 (a 20 bp unit x 200 with 2 % divergence): lists longer than 64 nodes run in the 400-slot kernel; the same
    reads under PHMM_WIDE_HINTED=1 PHMM_WIDE_EDGE_BWD=1 take the block, and the rows agree within 1e-9 absolute"""
    arrays, reads, _, _ = dataset("u20n200", 40)
    rng = np.random.default_rng(5)
    reads = [reads[int(i)][:400] for i in rng.choice(len(reads), 3, replace=False)]
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    with _knobs({}):
        mp, _ = gm.generate_mappings(rc, None, True)
        assert np.max(np.diff(mp.arrays()[0].astype(np.int64))) > 64
        run = _Run(gm, rc, mp)
        assert _ffi.last_call_stats(STATS_WIDE)[1] == 0
    _well_formed(run, 3, arrays.n_edges + arrays.n_nodes)
    _check_oracle_per_read(oracle, arrays, reads, rc, mp, run, "u20n200")
    with _knobs(BLOCK):
        wide = _Run(gm, rc, mp)
        ms, launches, cells = _ffi.last_call_stats(STATS_WIDE)
    assert launches > 0 and cells > 0, "the block did not run"
    worst = 0.0
    for r in range(3):
        worst = max(worst, float(np.max(np.abs(wide.u.key_freqs(r) - run.u.key_freqs(r)))))
    print(f"u20n200: block against the wave kernels max |d| {worst:.3e}; ln P {np.max(np.abs(wide.lf - run.lf)):.3e}")
    assert worst < 1e-9
    assert np.max(np.abs(wide.end_terms - run.end_terms)) < 1e-9


def test_short_reads_on_hand_built_lists(gpu_lib, oracle):
    """reads under 100 bases, where the Begin terms over b_init's every node are not 0: lists are the oracle's dense
    posteriors cut to a per-read width (one-base and two-base reads included)"""
    arrays, _ = small_dbg_model(300, 12, 0.01, seed=5, min_copy_num=1)
    om = oracle.Model(arrays)
    reads = D.sample_reads(arrays, 10 ** 9, 60, seed=11, max_reads=8)
    reads = [reads[0][:1], reads[1][:2], reads[2][:5]] + [r[: 20 + 9 * j] for j, r in enumerate(reads[3:])]
    widths = [3, 1, 8, 12, 2, 40, 70, 5]
    po, nd = [0], []
    for r, w in zip(reads, widths):
        m = om.run(r).to_mapping(w)
        for i in range(len(r)):
            nodes = m.nodes(i)
            nd.extend(nodes)
            po.append(po[-1] + len(nodes))
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    mp = D.Mappings.from_arrays(rc, np.array(po, dtype=np.uint64), np.array(nd, dtype=np.uint32))
    with _knobs({}):
        run = _Run(gm, rc, mp)
    _well_formed(run, len(reads), arrays.n_edges + arrays.n_nodes)
    big_end = _check_oracle_per_read(oracle, arrays, reads, rc, mp, run, "short reads")
    assert big_end > 1e-6, "the end terms were not exercised"


# ------------------------------------------------------------------ 3. against the summed call
def test_against_the_summed_call(gpu_lib, fix70):
    arrays, _, reads, gm, rc, mp, run = fix70
    E, N, R = arrays.n_edges, arrays.n_nodes, len(reads)
    with _knobs({}):
        lf, ef, inf = gm.run_with_mapping_edge_freqs(rc, mp)
    assert cc.same_bits(run.lf, lf), "out_logp_forward is not that of the summed call"
    pm, px = np.exp(arrays.param.p_match), np.exp(arrays.param.p_mismatch)
    ends = np.zeros(N)
    for r, read in enumerate(reads):
        e = np.where(arrays.emission == read[-1], pm, px)
        ends += np.exp(arrays.init_logp) * (run.end_terms[r, 0] + run.end_terms[r, 1] * e)
    d_e, d_i = np.max(np.abs(run.totals[:E] - ef)), np.max(np.abs(run.totals[E:] + ends - inf))
    print(f"against the summed call: max |d| edges {d_e:.3e}, init {d_i:.3e}")
    assert d_e < TOL_FREQ * R and d_i < TOL_FREQ * R
    # the totals are the column sums of the exported rows by the header's second rule, bit for bit
    want = _totals_by_the_rule(run)
    assert cc.same_bits(run.totals, want), np.flatnonzero(run.totals != want)[:10]
    assert np.all(run.totals[np.bincount(run.keys, minlength=E + N) == 0] == 0.0)


# ------------------------------------------------------------------ 4. independence and repeatability
def test_independence_and_repeatability(gpu_lib, fix70):
    arrays, _, reads, gm, rc, mp, full = fix70
    po, nd, lp = mp.arrays()
    off = rc.offsets.astype(np.int64)
    with _knobs({}):
        for r in (0, 17, 69):
            rc1 = D.ReadCollection([reads[r]])
            mp1 = D.Mappings.from_arrays(rc1, *subset_csr(off, (po, nd, lp), [r])[:2])
            one = _Run(gm, rc1, mp1)
            assert np.array_equal(one.u.row(0)[0], full.u.row(r)[0]) and cc.same_bits(one.u.row(0)[1], full.u.row(r)[1]), r
            assert one.lf[0] == full.lf[r] and cc.same_bits(one.end_terms[0], full.end_terms[r])
        again = _Run(gm, rc, mp)
        assert again.same_bits(full) and again.stats[1:] == full.stats[1:]


def test_output_forms(gpu_lib, fix70):
    """device-pointer outputs and a device export equal the host ones, every output may be NULL, out == NULL works, and
    a call without reads writes nothing and returns a handle of 0 rows"""
    arrays, _, reads, gm, rc, mp, full = fix70
    L = _ffi_edges.lib()
    R, K, T = len(reads), arrays.n_edges + arrays.n_nodes, int(full.keys.size)
    with _knobs({}):
        dl, de, dt = (cc.DeviceArray(8 * R, slack=cc.SLACK), cc.DeviceArray(16 * R, slack=cc.SLACK),
                      cc.DeviceArray(8 * K, slack=cc.SLACK))
        h = C.c_void_p()
        _ffi.check(L.phmm_run_with_mapping_read_edges(gm._h, rc._h, mp._h, 0, None, None, dl.p, de.p, dt.p, C.byref(h)))
        try:
            assert (L.phmm_read_edges_reads(h), L.phmm_read_edges_keys(h), L.phmm_read_edges_total(h)) == (R, K, T)
            assert cc.same_bits(dl.numpy(np.float64), full.lf) and cc.same_bits(dt.numpy(np.float64), full.totals)
            assert cc.same_bits(de.numpy(np.float64).reshape(R, 2), full.end_terms)
            assert all(np.all(d.bytes()[d.nbytes:] == cc.POISON) for d in (dl, de, dt))
            d_off, d_keys, d_use = (cc.DeviceArray(8 * (R + 1), slack=cc.SLACK), cc.DeviceArray(4 * T, slack=cc.SLACK),
                                    cc.DeviceArray(8 * T, slack=cc.SLACK))
            _ffi.check(L.phmm_read_edges_export(h, d_off.p, d_keys.p, d_use.p))
            assert np.array_equal(d_off.numpy(np.uint64), full.row_off) and np.array_equal(d_keys.numpy(np.uint32), full.keys)
            assert cc.same_bits(d_use.numpy(np.float64), full.usage)
            assert all(np.all(d.bytes()[d.nbytes:] == cc.POISON) for d in (d_off, d_keys, d_use))
            keys = np.zeros(T, dtype=np.uint32)
            _ffi.check(L.phmm_read_edges_export(h, None, P(keys), None))
            assert np.array_equal(keys, full.keys)
        finally:
            L.phmm_read_edges_destroy(h)
        # every output NULL; out == NULL with scores and totals; the handle alone
        _ffi.check(L.phmm_run_with_mapping_read_edges(gm._h, rc._h, mp._h, 0, None, None, None, None, None, None))
        lf, tot = np.full(R, 7.5), np.full(K, 7.5)
        _ffi.check(L.phmm_run_with_mapping_read_edges(gm._h, rc._h, mp._h, 0, None, None, P(lf), None, P(tot), None))
        assert cc.same_bits(tot, full.totals) and cc.same_bits(lf, full.lf)
        alone = _Run(gm, rc, mp, want_totals=False)
        assert alone.totals is None and np.array_equal(alone.keys, full.keys) and cc.same_bits(alone.usage, full.usage)
        # no reads: nothing is written, the handle has 0 rows
        rc0 = D.ReadCollection([])
        mp0 = D.Mappings.from_arrays(rc0, np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint32))
        lf, tot, et = np.full(1, 7.5), np.full(K, 7.5), np.full(2, 7.5)
        h = C.c_void_p()
        _ffi.check(L.phmm_run_with_mapping_read_edges(gm._h, rc0._h, mp0._h, 0, None, None, P(lf), P(et), P(tot), C.byref(h)))
        try:
            assert h.value and np.all(lf == 7.5) and np.all(tot == 7.5) and np.all(et == 7.5)
            assert (L.phmm_read_edges_reads(h), L.phmm_read_edges_keys(h), L.phmm_read_edges_total(h)) == (0, K, 0)
            row_off = np.full(1, 9, dtype=np.uint64)
            _ffi.check(L.phmm_read_edges_export(h, P(row_off), None, None))
            assert row_off.tolist() == [0]
        finally:
            L.phmm_read_edges_destroy(h)


# ------------------------------------------------------------------ 5. key maps
def test_link_keys_rows_are_the_default_rows_folded(gpu_lib, fix70):
    arrays, sg, reads, gm, rc, mp, full = fix70
    E = arrays.n_edges
    edge_key, links = D.link_keys(arrays, D.unitig_groups(sg))
    K = links.shape[0]
    assert K > 1 and np.any(edge_key == NO_KEY)
    with _knobs({}):
        run = _Run(gm, rc, mp, edge_key=edge_key, init_key=None, n_keys=K)
    _well_formed(run, len(reads), K)
    assert cc.same_bits(run.lf, full.lf) and cc.same_bits(run.end_terms, full.end_terms)
    worst, crossed = 0.0, 0
    for r, read in enumerate(reads):
        dk, du = full.u.row(r)
        sel = dk < E
        mk = edge_key[dk[sel]]
        keep = mk != NO_KEY
        want_keys, inv, m = np.unique(mk[keep], return_inverse=True, return_counts=True)
        want = np.zeros(want_keys.size)
        np.add.at(want, inv, du[sel][keep])
        gk, gu = run.u.row(r)
        assert np.array_equal(gk, want_keys), r
        n = 6.0 * (len(read) + 1) * m
        rel = np.abs(gu - want) / want
        worst = max(worst, float(np.max(rel / EPS)) if rel.size else 0.0)
        assert np.all(np.abs(gu - want) <= (n + 4) * EPS * want), r
        crossed += gk.size
    print(f"link keys: {K} links, {crossed} row entries, max |got - folded| / folded = {worst:.2f} * 2^-52")
    assert crossed > 0
    assert cc.same_bits(run.totals, _totals_by_the_rule(run))


def test_maps_that_leave_everything_out_and_keys_that_add(gpu_lib, fix70):
    arrays, _, reads, gm, rc, mp, full = fix70
    E, N, R = arrays.n_edges, arrays.n_nodes, len(reads)
    with _knobs({}):
        none = _Run(gm, rc, mp, edge_key=np.full(E, NO_KEY, dtype=np.uint32), init_key=None, n_keys=3)
        assert none.row_off.tolist() == [0] * (R + 1) and none.keys.size == 0 and np.all(none.totals == 0.0)
        assert none.totals.shape == (3,) and cc.same_bits(none.lf, full.lf)
        # two edges of one read on key 0, every Begin transition on key 1
        dk, du = full.u.row(0)
        e_a, e_b = int(dk[0]), int(dk[1])
        assert e_b < E
        ek = np.full(E, NO_KEY, dtype=np.uint32)
        ek[[e_a, e_b]] = 0
        two = _Run(gm, rc, mp, edge_key=ek, init_key=np.ones(N, dtype=np.uint32), n_keys=2)
    gk, gu = two.u.row(0)
    assert gk.tolist() == [0, 1]
    want = du[0] + du[1]
    assert abs(gu[0] - want) <= (6.0 * (len(reads[0]) + 1) * 2 + 4) * EPS * want
    begin = du[dk >= E]
    assert abs(gu[1] - begin.sum()) <= (6.0 * (len(reads[0]) + 1) * begin.size + 4) * EPS * begin.sum()
    for r in range(R):
        assert set(two.u.row(r)[0].tolist()) <= {0, 1}


# ------------------------------------------------------------------ 6. refusals
class _Prefilled:
    """outputs of a raw call, pre-filled, and a handle slot that holds a mark: a refusal leaves them as they are"""
    MARK = 0x1234560

    def __init__(self, n_reads, n_keys):
        self.lf, self.et, self.tot = np.full(max(n_reads, 1), 7.5), np.full((max(n_reads, 1), 2), 7.5), np.full(max(n_keys, 1), 7.5)
        self.h = C.c_void_p(self.MARK)

    def call(self, gm, rc, mp, n_keys=0, edge_key=None, init_key=None):
        return _ffi_edges.lib().phmm_run_with_mapping_read_edges(gm._h, rc._h, mp._h, n_keys, P(edge_key), P(init_key),
                                                                 P(self.lf), P(self.et), P(self.tot), C.byref(self.h))

    def untouched(self):
        return bool(np.all(self.lf == 7.5) and np.all(self.et == 7.5) and np.all(self.tot == 7.5) and self.h.value == self.MARK)


def test_refusals_of_the_edges_call(gpu_lib):
    """a model that cuts a read on its lists (a zero-copy k-mer) names the read; mappings of another read set are
    PHMM_EINVAL (the construction of tests/test_gpu_hinted_edges.py::test_refusals); *out is untouched"""
    arrays, sg = small_dbg_model(900, 12, 0.003, seed=21, min_copy_num=1)
    reads = [r for r in D.sample_reads(arrays, 10 ** 9, 420, seed=21, max_reads=40) if len(r) > 380][:4]
    rc = D.ReadCollection(reads)
    gm = D.PHMMModel(arrays)
    K = arrays.n_edges + arrays.n_nodes
    with _knobs({}):
        mp, _ = gm.generate_mappings(rc, None, True)
        ok = _Run(gm, rc, mp)
        assert np.all(np.isfinite(ok.lf))
        po, nd, _ = mp.arrays()
        p0 = int(rc.offsets[0])
        cn = sg.copy_num.copy()
        cn[np.unique(nd[int(po[p0 + 300]):int(po[p0 + 306])])] = 0
        with np.errstate(divide="ignore"):
            a2 = D.vectorised_to_phmm(D.SeqGraph(cn, sg.base, sg.edge_src, sg.edge_dst, None), arrays.param, 0)
        cut = D.PHMMModel(a2)
        out = _Prefilled(4, K)
        assert out.call(cut, rc, mp) == _ffi.PHMM_EINVAL and out.untouched()
        with pytest.raises(D.PhmmError, match="read 0"):
            cut.run_with_mapping_read_edges(rc, mp)
        other = D.ReadCollection(reads[:1])
        out = _Prefilled(4, K)
        assert out.call(gm, other, mp) == _ffi.PHMM_EINVAL and out.untouched()
    L = _ffi_edges.lib()
    for args in ((None, rc._h, mp._h), (gm._h, None, mp._h), (gm._h, rc._h, None)):
        assert L.phmm_run_with_mapping_read_edges(*args, 0, None, None, None, None, None, None) == _ffi.PHMM_EINVAL


def test_key_map_refusals(gpu_lib, fix70):
    arrays, _, reads, gm, rc, mp, full = fix70
    E, N, R = arrays.n_edges, arrays.n_nodes, len(reads)
    ek = np.zeros(E, dtype=np.uint32)
    with _knobs({}):
        out = _Prefilled(R, 4)
        assert out.call(gm, rc, mp, 4, None, None) == _ffi.PHMM_EINVAL and out.untouched(), "both maps NULL"
        bad = ek.copy()
        bad[E // 2] = 4
        assert out.call(gm, rc, mp, 4, bad, None) == _ffi.PHMM_EINVAL and out.untouched(), "edge_key value == n_keys"
        bad_i = np.full(N, NO_KEY, dtype=np.uint32)
        bad_i[N - 1] = 0xfffffffe
        assert out.call(gm, rc, mp, 4, ek, bad_i) == _ffi.PHMM_EINVAL and out.untouched(), "init_key value >= n_keys"
        with pytest.raises(D.PhmmError) as e:
            gm.run_with_mapping_read_edges(rc, mp, edge_key=bad, n_keys=4)
        assert e.value.code == _ffi.PHMM_EINVAL
        # and the call still works
        assert _Run(gm, rc, mp).same_bits(full)


def test_the_handle_outlives_its_inputs(gpu_lib):
    """exported after the model, the reads and the mappings are destroyed: the handle borrows nothing"""
    arrays, _, reads = _fixture_reads(5)
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    with _knobs({}):
        mp, _ = gm.generate_mappings(rc, None, True)
        want = _Run(gm, rc, mp)
        lf, u = gm.run_with_mapping_read_edges(rc, mp)
    del mp, rc, gm
    gc.collect()
    other = D.PHMMModel(D.mock_linear().to_phmm(D.PHMMParams.default()))  # (another model takes the device meanwhile)
    other.run(b"ATTCGTCGT")
    row_off, keys, usage = u.arrays()
    assert np.array_equal(row_off, want.row_off) and np.array_equal(keys, want.keys) and cc.same_bits(usage, want.usage)


# ------------------------------------------------------------------ 7. the caller contract
@pytest.fixture(scope="module")
def ctx(gpu_lib):
    return cc.Ctx()


@pytest.fixture(scope="module")
def scratch(gpu_lib):
    s = cc.DeviceArray(cc.SCRATCH_BYTES, 0)
    yield s
    s.free()


def _exported(L, h):
    R, T = L.phmm_read_edges_reads(h), L.phmm_read_edges_total(h)
    row_off, keys, usage = np.zeros(R + 1, dtype=np.uint64), np.zeros(max(T, 1), dtype=np.uint32), np.zeros(max(T, 1))
    _ffi.check(L.phmm_read_edges_export(h, P(row_off), P(keys), P(usage)))
    return {"row_off": row_off, "keys": keys[:T], "usage": usage[:T]}


def _row():
    """the new entry point as a row of caller_cases: the three output arrays where the caller wants them, the handle
    exported through the host-pointer form into extras"""
    L = _ffi_edges.lib()
    outs = lambda c: [cc.Out("logp_forward", cc.F8, (c.R,)), cc.Out("end_terms", cc.F8, (c.R, 2)),  # noqa: E731
                      cc.Out("key_usage", cc.F8, (c.E + c.N,))]

    def call(c, b):
        h = C.c_void_p()
        c.ffi.check(L.phmm_run_with_mapping_read_edges(c.gm._h, c.rc._h, c.mp._h, 0, None, None, b["logp_forward"],
                                                       b["end_terms"], b["key_usage"], C.byref(h)))
        try:
            return _exported(L, h)
        finally:
            L.phmm_read_edges_destroy(h)
    return cc.Row("run_with_mapping_read_edges", list(_ffi_edges.EDGES_SYMBOLS["phmm_amd_edges.h"]), outs, call)


def test_device_outputs_and_a_busy_stream(ctx, scratch):
    row = _row()
    want = cc.run_host(ctx, row)
    assert np.all(np.isfinite(want["logp_forward"])) and want["keys"].size > 0
    for stream in (None, cc.Stream()):
        d = cc.DeviceOutputs(ctx, row, stream)
        try:
            if stream is None:
                extras = row.call(ctx, d.pointers())
                got, clean = d.read()
            else:
                with cc.on_stream(ctx.lib, stream):
                    cc.queue_work(stream, scratch)
                    d.poison(stream)
                    busy = stream.query()
                    extras = row.call(ctx, d.pointers())
                    got, clean = d.read()
                assert busy == cc.HIP_ERROR_NOT_READY, "the queued work had drained before the call: the case ordered nothing"
            got.update(extras)
            assert not cc.same_result(want, got), cc.same_result(want, got)
            assert set(want) == set(got) and clean, "bytes behind an output's extent were written"
        finally:
            d.free()
            if stream is not None:
                stream.destroy()


def test_four_calls_do_not_grow_the_workspace(ctx):
    row = _row()
    runs, ws = [], []
    for _ in range(4):
        runs.append(cc.run_host(ctx, row))
        ws.append(ctx.lib.phmm_workspace_bytes())
    assert ws[1] == ws[2] == ws[3], ws
    for k in (1, 2, 3):
        assert not cc.same_result(runs[0], runs[k]), (k, cc.same_result(runs[0], runs[k]))
