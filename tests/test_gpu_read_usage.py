"""GPU: per-read node usage over mapping lists (phmm_run_with_mapping_read_usage, PHMMModel.run_with_mapping_read_usage,
include/phmm_amd_usage.h): PHMMOutput::to_state_probs() / to_node_freqs() (freq.rs:237-255) of every read on its lists,
as a sparse read-by-key matrix reduced on the device from the values of the states call.

Two bars, both derived.
  1. Against the restatement (read_usage_ref.py, math.fsum) on the call's OWN states values -- the same knobs, the values
     exported by run_with_mapping_states:  |got - ref| <= (n + 4) * 2^-52 * ref + n * 2^-1022, n the segment's term
     count.  exp is within 4 * 2^-52 on either side (the reasoning of test_gpu_mea_path.py), a sum of n non-negative
     doubles in any order adds at most (n - 1) * 2^-53 relative; the last part covers subnormal terms.
  2. Against the oracle (its to_emit_probs(p + 1) at the listed nodes, summed by the same restatement):
     |got - want| <= 1.01e-8 * want + 1.01e-12 * n: the bars of test_gpu_states.py carried through a sum -- a value at or
     above ln 1e-12 is within 1e-8 in the log, one below is only known to be smaller than 1e-12.
The structure (row_off, keys) and out_logp_forward are held bit for bit.

phmm_reads_create takes no empty read, so a read whose row is empty is here a read all of whose nodes are in no group."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import caller_cases as cc
import dbgphmm_amd as D
from dbgphmm_amd import _ffi, _ffi_usage
from helpers import small_dbg_model, subset_csr
from read_usage_ref import read_usage_ref
from repeat_cases import dataset

pytestmark = pytest.mark.gpu
EPS, TINY = 2.0 ** -52, 2.0 ** -1022
STATS_USAGE = 2
WIDTHS = (64, 65, 128, 129, 256, 257, 399, 400)
KNOBS = ("PHMM_WIDE_HINTED", "PHMM_NO_WIDE_HINTED", "PHMM_WIDE_STATES_BWD", "PHMM_WIDE_EDGE_BWD", "PHMM_NO_WIDE_LIST_BWD",
         "PHMM_WIDE_BWD_T")
BOTH = {"PHMM_WIDE_HINTED": "1", "PHMM_WIDE_STATES_BWD": "1"}
GENERIC = {"PHMM_NO_WIDE_HINTED": "1"}
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


def oracle_states(oracle, arrays, reads, rc, po, nd):
    """the oracle's run_with_mapping(read, its lists).to_emit_probs(p + 1) at the listed nodes -> want[entries, 3]"""
    om = oracle.Model(arrays)
    off = rc.offsets.astype(np.int64)
    po = po.astype(np.int64)
    want = np.full((int(po[-1]), 3), np.nan)
    with np.errstate(divide="ignore"):
        for i, r in enumerate(reads):
            o = om.run_with_mapping(r, oracle.Mapping(*subset_csr(off, (po.astype(np.uint64), nd, np.zeros(nd.size)), [i])))
            for p in range(len(r)):
                a0, a1 = int(po[off[i] + p]), int(po[off[i] + p + 1])
                m, ins, d, _ = o.to_emit_probs(p + 1)
                v = nd[a0:a1]
                want[a0:a1, 0], want[a0:a1, 1], want[a0:a1, 2] = m[v], ins[v], d[v]
    assert not np.any(np.isnan(want))
    return want


class _Run:
    """one run_with_mapping_read_usage call, its rows on the host, and index 2 of its statistics"""

    def __init__(self, gm, rc, mp, groups=None, want_totals=True):
        self.lf, self.u = gm.run_with_mapping_read_usage(rc, mp, groups, want_totals)
        self.stats = _ffi.last_call_stats(STATS_USAGE)
        self.row_off, self.keys, self.usage = self.u.arrays()
        self.totals = self.u.totals

    def same_bits(self, other):
        return all(cc.same_bits(np.asarray(a), np.asarray(b)) for a, b in
                   ((self.lf, other.lf), (self.row_off, other.row_off), (self.keys, other.keys), (self.usage, other.usage),
                    (self.totals, other.totals)))


def _bar1(got, ref, n):
    return np.abs(got - ref) <= (n + 4) * EPS * ref + n * TINY


def _bar2(got, want, n):
    return np.abs(got - want) <= 1.01e-8 * want + 1.01e-12 * n


def _hold(what, run, gm, rc, mp, groups=None, want_sl=None):
    """the run against the restatement on the states values of a call under the same knobs (bar 1, structure and ln P bit
    for bit), its totals against its own rows (bar 1), and -- with the oracle's values -- against the oracle (bar 2)"""
    po, nd, _ = mp.arrays()
    lf, sl, _ = gm.run_with_mapping_states(rc, mp, want_best=False)
    assert cc.same_bits(run.lf, lf), what + ": out_logp_forward is not that of the states call"
    row_off, keys, usage, totals, terms = read_usage_ref(rc.offsets, po, nd, sl, gm.n_nodes, groups)
    assert np.array_equal(run.row_off, row_off) and np.array_equal(run.keys, keys), what + ": structure"
    assert run.usage.shape == usage.shape and not np.any(np.isnan(run.usage))
    n = terms[:, None].astype(np.float64)
    ok = _bar1(run.usage, usage, n)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.nanmax(np.where(usage > 0, np.abs(run.usage - usage) / usage / EPS, 0.0)) if usage.size else 0.0
    print(f"{what}: {keys.size} row entries, segments of 1 .. {int(terms.max()) if terms.size else 0} terms, "
          f"max |got - ref| / ref = {rel:.2f} * 2^-52")
    assert np.all(ok), what + ": bar 1"
    if run.totals is not None:
        K = run.totals.shape[0]
        cols = [[[], [], []] for _ in range(K)]
        for k, row in zip(run.keys.tolist(), run.usage.tolist()):
            for s in range(3):
                cols[k][s].append(row[s])
        col_ref = np.array([[math.fsum(c[s]) for s in range(3)] for c in cols]).reshape(K, 3)
        col_n = np.bincount(run.keys, minlength=K).astype(np.float64)[:, None]
        assert np.all(_bar1(run.totals, col_ref, col_n)), what + ": totals are not the column sums of the rows"
        assert np.all(run.totals[col_n[:, 0] == 0] == 0.0)
        # (against the restatement's totals the rows' own error comes on top: every row within (n + 4) * 2^-52 of its
        # reference, n at most the longest segment, then the column sum of col_n terms)
        assert np.all(_bar1(run.totals, totals, col_n + n.max(initial=0.0))), what + ": totals against the restatement"
    if want_sl is not None:
        _, okeys, want, _, _ = read_usage_ref(rc.offsets, po, nd, want_sl, gm.n_nodes, groups)
        assert np.array_equal(okeys, keys)
        d = np.abs(run.usage - want)
        print(f"{what}: against the oracle max |d| {float(d.max()) if d.size else 0.0:.3e}")
        assert np.all(_bar2(run.usage, want, n)), what + ": bar 2"


def _groups_mod3(n_nodes):
    order = np.argsort(np.arange(n_nodes) % 3, kind="stable").astype(np.uint32)
    cnt = np.bincount(np.arange(n_nodes) % 3, minlength=3)
    return np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64), order


def _one_group(n_nodes):
    return np.array([0, n_nodes], dtype=np.uint64), np.arange(n_nodes, dtype=np.uint32)


# ------------------------------------------------------------------ 1. every node listed: the dense run
@pytest.mark.parametrize("which", ["zero_error", "default"])
def test_every_node_listed_is_the_dense_run(gpu_lib, oracle, which):
    """Fails without the feature: the call does not exist."""
    param, read = ((D.PHMMParams.zero_error(), b"CGATC") if which == "zero_error" else (D.PHMMParams.default(), b"ATTCGTCGT"))
    arrays = D.mock_linear().to_phmm(param)
    assert arrays.n_nodes == 10
    gm, rc = D.PHMMModel(arrays), D.ReadCollection([read])
    T = len(read)
    mp = D.Mappings.from_arrays(rc, np.arange(T + 1, dtype=np.uint64) * 10, np.tile(np.arange(10), T))
    po, nd, _ = mp.arrays()
    with np.errstate(divide="ignore"):
        want_sl = oracle_states(oracle, arrays, [read], rc, po, nd)
        run = _Run(gm, rc, mp)
        _hold(f"linear, {which}", run, gm, rc, mp, None, want_sl)
        want = oracle.Model(arrays).run(read).to_node_freqs()
        dense = gm.run(read).to_node_freqs()
    got = run.u.node_freqs(0)
    assert got.shape == (10,) and np.array_equal(run.keys, np.arange(10))
    # (M + I + D per node: three sums of T terms each)
    assert np.all(_bar2(got, want, 3.0 * T)), (got, want)
    assert np.all(_bar2(got, dense, 3.0 * T)), (got, dense)
    assert np.all(_bar2(run.u.state_probs(0).sum(axis=1), want, 3.0 * T))
    assert run.stats[2] == int(po[-1])  # cells = list entries


# ------------------------------------------------------------------ 2. generated lists
def _fixture_reads(n):
    arrays, _ = small_dbg_model(300, 12, 0.01, seed=5)
    reads = D.sample_reads(arrays, 10 ** 9, 60, seed=70, max_reads=70)
    assert len(reads) == 70
    return arrays, [r[: max(1, len(r) - (j * 7) % 31)] for j, r in enumerate(reads)][:n]


@pytest.fixture(scope="module")
def fix70(gpu_lib, oracle):
    arrays, reads = _fixture_reads(70)
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    with _knobs({}):
        mp, _ = gm.generate_mappings(rc, None, True)
        po, nd, _ = mp.arrays()
        run = _Run(gm, rc, mp)
    return arrays, reads, gm, rc, mp, oracle_states(oracle, arrays, reads, rc, po, nd), run


@pytest.mark.parametrize("n_reads", [1, 5, 70])
def test_generated_lists(gpu_lib, oracle, fix70, n_reads):
    if n_reads == 70:
        arrays, reads, gm, rc, mp, want_sl, run = fix70
    else:
        arrays, reads = _fixture_reads(n_reads)
        gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
        with _knobs({}):
            mp, _ = gm.generate_mappings(rc, None, True)
            run = _Run(gm, rc, mp)
        want_sl = oracle_states(oracle, arrays, reads, rc, *mp.arrays()[:2])
    with _knobs({}):
        _hold(f"generated lists, {n_reads} reads", run, gm, rc, mp, None, want_sl)
    po = mp.arrays()[0]
    assert run.stats[1] > 0 and run.stats[2] == int(po[-1])
    assert len(run.u) == n_reads and run.u.n_keys == arrays.n_nodes and run.totals.shape == (arrays.n_nodes, 3)
    per_base = run.keys.size / rc.total_bases()
    print(f"generated lists, {n_reads} reads: {per_base:.2f} keys per base")
    # reads_of is the transpose of row
    for key in np.unique(run.keys)[:: max(1, np.unique(run.keys).size // 25)].tolist():
        rd, us = run.u.reads_of(key)
        want_rd = [r for r in range(n_reads) if key in run.u.row(r)[0]]
        assert rd.tolist() == want_rd
        for r, x in zip(rd.tolist(), us):
            keys, usage = run.u.row(r)
            assert np.array_equal(usage[np.searchsorted(keys, key)], x)
    assert run.u.reads_of(arrays.n_nodes - 1)[0].size == int(np.sum(run.keys == arrays.n_nodes - 1))


# ------------------------------------------------------------------ 3. groups
@pytest.mark.parametrize("kind", ["mod3", "singletons_shuffled", "odd_ungrouped", "empty_group", "one_group"])
def test_groups(gpu_lib, fix70, kind):
    arrays, reads, gm, rc, mp, want_sl, node_run = fix70
    N = arrays.n_nodes
    rng = np.random.default_rng(31)
    if kind == "mod3":
        groups = _groups_mod3(N)
    elif kind == "singletons_shuffled":
        groups = (np.arange(N + 1, dtype=np.uint64), rng.permutation(N).astype(np.uint32))
    elif kind == "odd_ungrouped":
        even = np.arange(0, N, 2, dtype=np.uint32)
        groups = (np.arange(even.size + 1, dtype=np.uint64), even)
    elif kind == "empty_group":
        a, b = np.arange(0, N, 4, dtype=np.uint32), np.arange(1, N, 4, dtype=np.uint32)
        groups = (np.array([0, 0, a.size, a.size, a.size + b.size, a.size + b.size], dtype=np.uint64), np.concatenate([a, b]))
    else:
        groups = _one_group(N)
    with _knobs({}):
        run = _Run(gm, rc, mp, groups)
        _hold(f"groups, {kind}", run, gm, rc, mp, groups, want_sl)
    K = groups[0].size - 1
    assert run.u.n_keys == K and run.totals.shape == (K, 3)
    if kind == "mod3":
        seg = np.array([np.sum(mp.arrays()[1][int(mp.arrays()[0][rc.offsets[r]]):int(mp.arrays()[0][rc.offsets[r + 1]])] % 3 == 0)
                        for r in range(len(reads))])
        print(f"groups, mod3: segments of group 0 hold {seg.min()} .. {seg.max()} entries")
        assert seg.min() <= 64 < seg.max()  # both classes of the reduction
    if kind == "singletons_shuffled":  # group g is node groups[1][g] alone: the node rows under other names, bit for bit
        name = np.empty(N, dtype=np.int64)
        name[groups[1]] = np.arange(N)
        for r in range(len(reads)):
            nk, nu = node_run.u.row(r)
            gk, gu = run.u.row(r)
            order = np.argsort(name[nk])
            assert np.array_equal(gk, name[nk][order]) and cc.same_bits(gu, nu[order])
    if kind == "empty_group":
        assert set(np.unique(run.keys).tolist()) <= {1, 3} and np.all(run.totals[[0, 2, 4]] == 0.0)
    if kind == "one_group":
        assert np.array_equal(run.row_off, np.arange(len(reads) + 1)) and np.all(run.keys == 0)


# ------------------------------------------------------------------ 4. boundary widths
def pad_lists(po, nd, reads, n_nodes, seed=5):
    """(of test_gpu_states.py, restated) the list of read j at two of every three positions padded with distinct other
    nodes, in shuffled order, to width WIDTHS[j % 8]; every third position keeps its own short list -> (pos_off, nodes)"""
    rng = np.random.default_rng(seed)
    out_off, out = [0], []
    g = 0
    for j, r in enumerate(reads):
        w = WIDTHS[j % 8]
        for i in range(len(r)):
            own = nd[int(po[g]):int(po[g + 1])]
            if i % 3 != 2 and own.size < w:
                others = np.setdiff1d(np.arange(n_nodes, dtype=np.uint32), own)
                lst = np.concatenate([own, rng.choice(others, size=w - own.size, replace=False).astype(np.uint32)])
                rng.shuffle(lst)
            else:
                lst = own
            out.append(lst)
            out_off.append(out_off[-1] + lst.size)
            g += 1
    return np.array(out_off, np.uint64), np.concatenate(out).astype(np.uint32)


@pytest.fixture(scope="module")
def crafted(gpu_lib, oracle):
    arrays, _ = small_dbg_model(600, 12, 0.01, seed=3)
    reads = D.sample_reads(arrays, 10 ** 9, 120, seed=4, max_reads=24)
    assert arrays.n_nodes == 740 and len(reads) == 24
    (po, nd, lp), _ = oracle.Model(arrays).generate_mappings(reads, None, True, n_threads=8)
    ppo, pnd = pad_lists(po, nd, reads, arrays.n_nodes)
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    return arrays, reads, gm, rc, D.Mappings.from_arrays(rc, ppo, pnd)


@pytest.mark.parametrize("setting", [{}, GENERIC, BOTH], ids=["default", "generic", "block"])
def test_boundary_widths(crafted, setting):
    arrays, reads, gm, rc, mp = crafted
    po = mp.arrays()[0].astype(np.int64)
    off = rc.offsets.astype(np.int64)
    per_read = po[off[1:]] - po[off[:-1]]
    with _knobs(setting):
        run = _Run(gm, rc, mp)
        _hold("crafted widths, node keys", run, gm, rc, mp)
        one = _Run(gm, rc, mp, _one_group(arrays.n_nodes))
        _hold("crafted widths, one group", one, gm, rc, mp, _one_group(arrays.n_nodes))
    # with one group of all nodes a read is one segment of all of its entries: 80 padded positions of 400 nodes and more
    assert np.array_equal(one.row_off, np.arange(len(reads) + 1))
    assert int(per_read.max()) > 30000 and int(per_read.min()) > 64
    assert cc.same_bits(one.lf, run.lf)


# ------------------------------------------------------------------ 5. seams
def test_seams(gpu_lib, fix70):
    arrays, reads, gm, rc, mp, _, full = fix70
    N = arrays.n_nodes
    po, nd, _ = mp.arrays()
    off = rc.offsets.astype(np.int64)
    pick = [3, 3, 7, 3]  # the same read twice in a row, and once more behind another
    rc2 = D.ReadCollection([reads[j] for j in pick])
    spo, snd, _ = subset_csr(off, (po, nd, np.zeros(nd.size)), pick)
    mp2 = D.Mappings.from_arrays(rc2, spo, snd)
    with _knobs({}):
        run = _Run(gm, rc2, mp2)
        _hold("seams", run, gm, rc2, mp2)
        rows = [run.u.row(r) for r in range(4)]
        assert run.row_off[1] - run.row_off[0] == run.row_off[2] - run.row_off[1] > 0  # two rows, not one merged segment
        for r in (1, 3):
            assert np.array_equal(rows[r][0], rows[0][0]) and cc.same_bits(rows[r][1], rows[0][1])
        want3, want7 = full.u.row(3), full.u.row(7)
        assert np.array_equal(rows[0][0], want3[0]) and cc.same_bits(rows[0][1], want3[1])
        assert np.array_equal(rows[2][0], want7[0]) and cc.same_bits(rows[2][1], want7[1])
        # reads whose rows are empty, in front, in the middle and at the end: only the nodes of read 7 alone are grouped
        only7 = np.setdiff1d(np.unique(snd[int(spo[2 * len(reads[3])]):int(spo[2 * len(reads[3]) + len(reads[7])])]),
                             np.unique(snd[:int(spo[len(reads[3])])])).astype(np.uint32)
        assert only7.size > 0
        groups = (np.array([0, only7.size], dtype=np.uint64), only7)
        part = _Run(gm, rc2, mp2, groups)
        _hold("seams, rows that are empty", part, gm, rc2, mp2, groups)
        assert part.row_off.tolist() == [0, 0, 0, 1, 1]
        nothing = _Run(gm, rc2, mp2, (np.array([0, 0], dtype=np.uint64), np.zeros(0, dtype=np.uint32)))
        assert nothing.row_off.tolist() == [0] * 5 and nothing.keys.size == 0 and np.all(nothing.totals == 0.0)
        assert cc.same_bits(nothing.lf, run.lf)


@pytest.mark.parametrize("setting", [GENERIC, BOTH], ids=["generic", "block"])
def test_a_node_that_leaves_the_list(gpu_lib, setting):
    """(fixture 6 of test_gpu_states.py) every other position p < len-1 of every read gets, at the head of its list, a node
    that list p+1 does not hold: its values are -inf, its terms exact zeros, and its key stays in the row"""
    arrays, _ = small_dbg_model(300, 12, 0.01, seed=5)
    reads = D.sample_reads(arrays, 10 ** 9, 60, seed=5, max_reads=5)
    rc = D.ReadCollection(reads)
    gm = D.PHMMModel(arrays)
    with _knobs({}):
        po, nd, _ = gm.generate_mappings(rc, None, True)[0].arrays()
    po = po.astype(np.int64)
    off = rc.offsets.astype(np.int64)
    rng = np.random.default_rng(6)
    new_off, new, gone = [0], [], []
    for i, r in enumerate(reads):
        read_nodes = np.unique(nd[po[off[i]]:po[off[i + 1]]])
        for p in range(len(r)):
            g = off[i] + p
            own = nd[po[g]:po[g + 1]]
            lst = own
            if i == 0 and p % 3 == 0:
                others = np.setdiff1d(np.arange(arrays.n_nodes, dtype=np.uint32), own)
                lst = np.concatenate([own, rng.choice(others, size=70 - own.size, replace=False).astype(np.uint32)])
            if p % 2 == 0 and p + 1 < len(r):
                nxt = nd[po[g + 1]:po[g + 2]]
                pool = np.setdiff1d(np.arange(arrays.n_nodes, dtype=np.uint32), np.concatenate([lst, nxt]))
                gone.append((i, new_off[-1]))
                lst = np.concatenate([[rng.choice(pool)], lst]).astype(np.uint32)
            new.append(lst)
            new_off.append(new_off[-1] + lst.size)
    npo, nnd = np.array(new_off, np.uint64), np.concatenate(new).astype(np.uint32)
    mp = D.Mappings.from_arrays(rc, npo, nnd)
    with _knobs(setting):
        run = _Run(gm, rc, mp)
        _hold("a node leaves the list", run, gm, rc, mp)
        _, sl, _ = gm.run_with_mapping_states(rc, mp, want_best=False)
    assert len(gone) > 100 and all(np.all(sl[a] == -np.inf) for _, a in gone)
    # a key all of whose terms are such entries stays in its row, with exact zeros
    zeros = 0
    for i in range(len(reads)):
        e0, e1 = int(npo[off[i]]), int(npo[off[i + 1]])
        dead = np.all(sl[e0:e1] == -np.inf, axis=1)
        for v in np.unique(nnd[e0:e1][dead]).tolist():
            if np.all(dead[nnd[e0:e1] == v]):
                keys, usage = run.u.row(i)
                j = int(np.searchsorted(keys, v))
                assert keys[j] == v and np.all(usage[j] == 0.0) and not np.any(np.signbit(usage[j]))
                zeros += 1
    print(f"a node leaves the list: {zeros} row entries of exact zeros")
    assert zeros > 20


# ------------------------------------------------------------------ 6. real wide lists
def test_real_wide_lists_u20(gpu_lib, oracle):
    arrays, reads, _, _ = dataset("u20", 40, max_reads=24)
    assert len(reads) == 24
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    with _knobs({}):
        mp, _ = gm.generate_mappings(rc, None, True)
        po, nd, _ = mp.arrays()
        want_sl = oracle_states(oracle, arrays, reads, rc, po, nd)
        run = _Run(gm, rc, mp)
        _hold("u20", run, gm, rc, mp, None, want_sl)
    seg = np.diff(run.row_off.astype(np.int64))
    print(f"u20: {int(po[-1])} entries, {run.keys.size} row entries, rows of {seg.min()} .. {seg.max()} keys")


# ------------------------------------------------------------------ 7. independence
def test_independence(gpu_lib, fix70):
    arrays, reads, gm, rc, mp, _, full = fix70
    po, nd, _ = mp.arrays()
    off = rc.offsets.astype(np.int64)
    with _knobs({}):
        # the rows of reads [3, 7] called alone
        rc2 = D.ReadCollection([reads[3], reads[7]])
        mp2 = D.Mappings.from_arrays(rc2, *subset_csr(off, (po, nd, np.zeros(nd.size)), [3, 7])[:2])
        two = _Run(gm, rc2, mp2)
        for j, r in enumerate((3, 7)):
            assert np.array_equal(two.u.row(j)[0], full.u.row(r)[0]) and cc.same_bits(two.u.row(j)[1], full.u.row(r)[1])
            assert two.lf[j] == full.lf[r]
        # a second call
        again = _Run(gm, rc, mp)
        assert again.same_bits(full) and again.stats[1:] == full.stats[1:]
        # under a workspace limit that holds the plane and the scratch of two of the longest reads (the header: 32 bytes
        # per list entry of a chunk and about 12 of the sort's own): three chunks at the least
        per_read = (po[off[1:]].astype(np.int64) - po[off[:-1]].astype(np.int64))
        n_ent = int(po[-1])
        assert n_ent > 2 * (2 * int(per_read.max()))
        _ffi.check(gpu_lib.phmm_set_workspace_limit(24 * n_ent + 44 * 2 * int(per_read.max()) + (64 << 10)))
        try:
            split = _Run(gm, rc, mp)
        finally:
            _ffi.check(gpu_lib.phmm_set_workspace_limit(0))
        print(f"independence: launches {full.stats[1]} unsplit, {split.stats[1]} under the limit")
        assert split.same_bits(full) and split.stats[1] > full.stats[1] and split.stats[2] == n_ent
        grouped = _Run(gm, rc, mp, _groups_mod3(arrays.n_nodes))
        _ffi.check(gpu_lib.phmm_set_workspace_limit(24 * n_ent + 44 * 2 * int(per_read.max()) + (64 << 10)))
        try:
            assert _Run(gm, rc, mp, _groups_mod3(arrays.n_nodes)).same_bits(grouped)
            # the plane alone does not fit: refused as the MEA call refuses
            _ffi.check(gpu_lib.phmm_set_workspace_limit(24 * n_ent - 8))
            with pytest.raises(D.PhmmError) as e:
                gm.run_with_mapping_read_usage(rc, mp)
            assert e.value.code == _ffi.PHMM_ECAPACITY
        finally:
            _ffi.check(gpu_lib.phmm_set_workspace_limit(0))


def test_output_forms(gpu_lib, fix70):
    """device-pointer outputs and a device export equal the host ones, every output may be NULL, and a call without reads
    writes nothing and returns a handle of 0 rows"""
    arrays, reads, gm, rc, mp, _, full = fix70
    L = _ffi_usage.lib()
    R, K, T = len(reads), arrays.n_nodes, int(full.keys.size)
    with _knobs({}):
        dl, dt = cc.DeviceArray(8 * R, slack=cc.SLACK), cc.DeviceArray(24 * K, slack=cc.SLACK)
        h = C.c_void_p()
        _ffi.check(L.phmm_run_with_mapping_read_usage(gm._h, rc._h, mp._h, 0, None, None, dl.p, dt.p, C.byref(h)))
        try:
            assert (L.phmm_read_usage_reads(h), L.phmm_read_usage_keys(h), L.phmm_read_usage_total(h)) == (R, K, T)
            assert cc.same_bits(dl.numpy(np.float64), full.lf) and cc.same_bits(dt.numpy(np.float64).reshape(K, 3), full.totals)
            assert np.all(dl.bytes()[8 * R:] == cc.POISON) and np.all(dt.bytes()[24 * K:] == cc.POISON)
            d_off, d_keys, d_use = (cc.DeviceArray(8 * (R + 1), slack=cc.SLACK), cc.DeviceArray(4 * T, slack=cc.SLACK),
                                    cc.DeviceArray(24 * T, slack=cc.SLACK))
            _ffi.check(L.phmm_read_usage_export(h, d_off.p, d_keys.p, d_use.p))
            assert np.array_equal(d_off.numpy(np.uint64), full.row_off) and np.array_equal(d_keys.numpy(np.uint32), full.keys)
            assert cc.same_bits(d_use.numpy(np.float64).reshape(T, 3), full.usage)
            assert all(np.all(d.bytes()[d.nbytes:] == cc.POISON) for d in (d_off, d_keys, d_use))
            # parts of the export
            keys = np.zeros(T, dtype=np.uint32)
            _ffi.check(L.phmm_read_usage_export(h, None, P(keys), None))
            assert np.array_equal(keys, full.keys)
        finally:
            L.phmm_read_usage_destroy(h)
        # every output NULL; out == NULL with the totals alone; the handle alone
        _ffi.check(L.phmm_run_with_mapping_read_usage(gm._h, rc._h, mp._h, 0, None, None, None, None, None))
        tot = np.full((K, 3), 7.5)
        _ffi.check(L.phmm_run_with_mapping_read_usage(gm._h, rc._h, mp._h, 0, None, None, None, P(tot), None))
        assert cc.same_bits(tot, full.totals)
        alone = _Run(gm, rc, mp, None, want_totals=False)
        assert alone.totals is None and np.array_equal(alone.keys, full.keys) and cc.same_bits(alone.usage, full.usage)
        # no reads: nothing is written, the handle has 0 rows
        rc0 = D.ReadCollection([])
        mp0 = D.Mappings.from_arrays(rc0, np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint32))
        lf, tot = np.full(1, 7.5), np.full((K, 3), 7.5)
        h = C.c_void_p()
        _ffi.check(L.phmm_run_with_mapping_read_usage(gm._h, rc0._h, mp0._h, 0, None, None, P(lf), P(tot), C.byref(h)))
        try:
            assert h.value and np.all(lf == 7.5) and np.all(tot == 7.5)
            assert (L.phmm_read_usage_reads(h), L.phmm_read_usage_keys(h), L.phmm_read_usage_total(h)) == (0, K, 0)
            row_off = np.full(1, 9, dtype=np.uint64)
            _ffi.check(L.phmm_read_usage_export(h, P(row_off), None, None))
            assert row_off.tolist() == [0]
        finally:
            L.phmm_read_usage_destroy(h)
        lf0, u0 = gm.run_with_mapping_read_usage(rc0, mp0)
        assert lf0.size == 0 and len(u0) == 0 and u0.arrays()[1].size == 0 and np.all(u0.totals == 0.0)


# ------------------------------------------------------------------ 8. refusals
class _Prefilled:
    """outputs of a raw call, pre-filled, and a handle slot that holds a mark: a refusal leaves them as they are"""
    MARK = 0x1234560

    def __init__(self, n_reads, n_keys):
        self.lf, self.tot = np.full(max(n_reads, 1), 7.5), np.full((max(n_keys, 1), 3), 7.5)
        self.h = C.c_void_p(self.MARK)

    def call(self, gm, rc, mp, groups=None, n_groups=None):
        g_off, g_nodes = (None, None) if groups is None else groups
        n = n_groups if n_groups is not None else (0 if g_off is None else g_off.size - 1)
        return _ffi_usage.lib().phmm_run_with_mapping_read_usage(gm._h, rc._h, mp._h, n, P(g_off), P(g_nodes), P(self.lf),
                                                                 P(self.tot), C.byref(self.h))

    def untouched(self):
        return bool(np.all(self.lf == 7.5) and np.all(self.tot == 7.5) and self.h.value == self.MARK)


def test_refusals_of_the_states_call(gpu_lib, crafted):
    arrays, reads, gm, rc_all, mp_all = crafted
    ppo, pnd, _ = mp_all.arrays()
    rc2 = D.ReadCollection(reads[:2])
    n = len(reads[0]) + len(reads[1])
    # every node listed at bases 100..105 of read 7 (lists of 400 nodes) goes to copy number 0: the read is cut there
    _, sg = small_dbg_model(600, 12, 0.01, seed=3)
    p0 = int(rc_all.offsets[7])
    cn = sg.copy_num.copy()
    cn[np.unique(pnd[int(ppo[p0 + 100]):int(ppo[p0 + 106])])] = 0
    with np.errstate(divide="ignore"):
        a2 = D.vectorised_to_phmm(D.SeqGraph(cn, sg.base, sg.edge_src, sg.edge_dst, None), arrays.param, 0)
    cut = D.PHMMModel(a2)

    def list_of_401(out):  # (refused where the lists are handed over, as for the states call)
        try:
            over = D.Mappings.from_arrays(rc2, np.arange(n + 1, dtype=np.uint64) * 401, np.tile(np.arange(401, dtype=np.uint32), n))
        except D.PhmmError as e:
            return e.code
        return out.call(gm, rc2, over)

    for setting in (BOTH, GENERIC):
        with _knobs(setting):
            outs = [_Prefilled(2, 740), _Prefilled(2, 740), _Prefilled(24, 740)]
            got = (outs[0].call(gm, rc2, mp_all), list_of_401(outs[1]), outs[2].call(cut, rc_all, mp_all))
            assert got == (_ffi.PHMM_EINVAL, _ffi.PHMM_ECAPACITY, _ffi.PHMM_EINVAL), got
            assert all(o.untouched() for o in outs)
    L = _ffi_usage.lib()
    for args in ((None, rc2._h, mp_all._h), (gm._h, None, mp_all._h), (gm._h, rc2._h, None)):
        assert L.phmm_run_with_mapping_read_usage(*args, 0, None, None, None, None, None) == _ffi.PHMM_EINVAL


def test_group_refusals(gpu_lib, fix70):
    arrays, reads, gm, rc, mp, _, full = fix70
    N = arrays.n_nodes
    u64, u32 = (lambda *a: np.array(a, dtype=np.uint64)), (lambda *a: np.array(a, dtype=np.uint32))
    bad = {
        "offsets not starting at 0": (u64(1, 2), u32(0, 1)),
        "offsets decreasing": (u64(0, 2, 1), u32(0, 1, 2)),
        "a node id >= N": (u64(0, 2), u32(0, N)),
        "a node in two groups": (u64(0, 2, 4), u32(0, 1, 1, 2)),
        "a node twice in one group": (u64(0, 3), u32(4, 5, 4)),
        "more entries than nodes": (u64(0, N + 1), np.arange(N + 1, dtype=np.uint32) % N),
    }
    with _knobs({}):
        for what, groups in bad.items():
            out = _Prefilled(len(reads), groups[0].size - 1)
            assert out.call(gm, rc, mp, groups) == _ffi.PHMM_EINVAL and out.untouched(), what
        # NULL arrays with n_groups > 0
        out = _Prefilled(len(reads), 2)
        assert out.call(gm, rc, mp, None, n_groups=2) == _ffi.PHMM_EINVAL and out.untouched()
        assert out.call(gm, rc, mp, (u64(0, 1, 2), None)) == _ffi.PHMM_EINVAL and out.untouched()
        # and the call still works
        assert _Run(gm, rc, mp).same_bits(full)


# ------------------------------------------------------------------ 9. the caller contract
@pytest.fixture(scope="module")
def ctx(gpu_lib):
    return cc.Ctx()


@pytest.fixture(scope="module")
def scratch(gpu_lib):
    s = cc.DeviceArray(cc.SCRATCH_BYTES, 0)
    yield s
    s.free()


def _row(keep=None):
    """the new entry point as a row of caller_cases: the two output arrays where the caller wants them, the handle
    exported through the host-pointer form into extras (or kept in `keep`, for the caller to export and destroy)"""
    L = _ffi_usage.lib()
    outs = lambda c: [cc.Out("logp_forward", cc.F8, (c.R,)), cc.Out("key_usage", cc.F8, (c.N, 3))]  # noqa: E731

    def call(c, b):
        h = C.c_void_p()
        c.ffi.check(L.phmm_run_with_mapping_read_usage(c.gm._h, c.rc._h, c.mp._h, 0, None, None, b["logp_forward"],
                                                       b["key_usage"], C.byref(h)))
        if keep is not None:
            keep.append(h)
            return {}
        try:
            return _exported(L, h)
        finally:
            L.phmm_read_usage_destroy(h)
    return cc.Row("run_with_mapping_read_usage", list(_ffi_usage.USAGE_SYMBOLS["phmm_amd_usage.h"]), outs, call)


def _exported(L, h):
    R, T = L.phmm_read_usage_reads(h), L.phmm_read_usage_total(h)
    row_off, keys, usage = np.zeros(R + 1, dtype=np.uint64), np.zeros(max(T, 1), dtype=np.uint32), np.zeros((max(T, 1), 3))
    _ffi.check(L.phmm_read_usage_export(h, P(row_off), P(keys), P(usage)))
    return {"row_off": row_off, "keys": keys[:T], "usage": usage[:T]}


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


def test_two_streams_alternating(ctx):
    row = _row()
    want = cc.run_host(ctx, row)
    streams = [cc.Stream(), cc.Stream()]
    try:
        for k in range(4):
            with cc.on_stream(ctx.lib, streams[k % 2]):
                got = cc.run_host(ctx, row)
            assert not cc.same_result(want, got), (k, cc.same_result(want, got))
    finally:
        for s in streams:
            s.destroy()


def test_four_calls_do_not_grow_the_workspace(ctx):
    row = _row()
    runs, ws = [], []
    for _ in range(4):
        runs.append(cc.run_host(ctx, row))
        ws.append(ctx.lib.phmm_workspace_bytes())
    assert ws[1] == ws[2] == ws[3], ws
    for k in (1, 2, 3):
        assert not cc.same_result(runs[0], runs[k]), (k, cc.same_result(runs[0], runs[k]))


def test_the_handle_outlives_its_inputs(gpu_lib):
    """exported after the model, the reads and the mappings are destroyed: the handle borrows nothing"""
    arrays, reads = _fixture_reads(5)
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    with _knobs({}):
        mp, _ = gm.generate_mappings(rc, None, True)
        want = _Run(gm, rc, mp)
        lf, u = gm.run_with_mapping_read_usage(rc, mp)
    del mp, rc, gm
    import gc
    gc.collect()
    other = D.PHMMModel(D.mock_linear().to_phmm(D.PHMMParams.default()))  # (another model takes the device meanwhile)
    other.run(b"ATTCGTCGT")
    row_off, keys, usage = u.arrays()
    assert np.array_equal(row_off, want.row_off) and np.array_equal(keys, want.keys) and cc.same_bits(usage, want.usage)
