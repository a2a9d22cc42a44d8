"""GPU: the backward half of phmm_run_with_mapping_edges on a block (wide_backward_kernel<true, true>, wide_bwd_kernel.h)
for reads whose longest mapping list holds 65-400 nodes, and the 128-thread size of the list backward's block.

Everything goes through the C ABI (PHMMModel.run_with_mapping_edge_freqs, generate_mappings) and is held to the oracle's
run_with_mapping(read, its lists).to_edge_and_init_freqs() summed over the reads.  Knobs: PHMM_WIDE_HINTED=1 puts the
forward half on a block, PHMM_WIDE_EDGE_BWD=1 beside it the edge-term backward, PHMM_NO_WIDE_LIST_BWD=1 holds the backward
to the generic kernel, PHMM_NO_WIDE_HINTED=1 both halves; PHMM_WIDE_BWD_T=128 / 448 chooses the backward block's size for
reads with lists of at most 128 nodes.  Every test sets the knobs it wants and clears the others.  pad_lists and the
crafted inputs are those of test_gpu_list_pass_wide.py (restated: a test module cannot be imported without editing it).

Tolerances: edge / init frequencies and ln P against the oracle, and between block and generic runs, 1e-9 x reads
(test_gpu_hinted_edges.py); ln P between kernels 1e-9."""
import os

import numpy as np
import pytest

import dbgphmm_amd as D
from dbgphmm_amd import _ffi
from graph_cases import zoo_graph, zoo_model
from helpers import small_dbg_model, subset_csr
from repeat_cases import dataset

pytestmark = pytest.mark.gpu
WIDTHS = (64, 65, 128, 129, 256, 257, 399, 400)
STATS_WIDE = 4
TOL_LOGP = 1e-9  # ln P per read between kernels
TOL_FREQ = 1e-9  # edge / init frequencies and ln P, times the number of reads (test_gpu_hinted_edges.py)
KNOBS = ("PHMM_WIDE_HINTED", "PHMM_NO_WIDE_HINTED", "PHMM_WIDE_EDGE_BWD", "PHMM_NO_WIDE_LIST_BWD", "PHMM_WIDE_BWD_T")
BOTH = {"PHMM_WIDE_HINTED": "1", "PHMM_WIDE_EDGE_BWD": "1"}
FWD_ONLY = {"PHMM_WIDE_HINTED": "1"}
GENERIC = {"PHMM_NO_WIDE_HINTED": "1"}


class _knobs:
    """exactly these knobs for the calls inside the block (knobs are read when a call takes the device)"""

    def __init__(self, setting, **more):
        self.setting = dict(setting, **more)

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


def _wide_stats():
    ms, launches, cells = _ffi.last_call_stats(STATS_WIDE)
    return launches, cells


def _read_max(rc, po):
    off, cnt = rc.offsets.astype(np.int64), np.diff(po.astype(np.int64))
    return np.array([cnt[off[r]:off[r + 1]].max() if off[r + 1] > off[r] else 0 for r in range(len(rc))])


def _entries(rc, po, which):
    off = rc.offsets.astype(np.int64)
    return int(sum(int(po[off[r + 1]]) - int(po[off[r]]) for r in np.flatnonzero(which)))


class _Edges:
    """what one run_with_mapping_edge_freqs(rc, mp) call returned, and index 4 of its statistics"""

    def __init__(self, gm, rc, mp, setting, **more):
        with _knobs(setting, **more):
            lf, ef, inf = gm.run_with_mapping_edge_freqs(rc, mp)
            self.stats = _wide_stats()
        self.lf, self.ef, self.inf = lf.copy(), ef.copy(), inf.copy()

    def same_bits(self, other):
        return np.array_equal(self.lf, other.lf) and np.array_equal(self.ef, other.ef) and np.array_equal(self.inf, other.inf)

    def dev(self, lf, ef, inf):
        return [float(np.max(np.abs(a - b))) if a.size else 0.0 for a, b in ((self.lf, lf), (self.ef, ef), (self.inf, inf))]


class _Lists:
    """what one generate_mappings(rc, mp, True) call returned, and index 4 of its statistics"""

    def __init__(self, gm, rc, mp, setting, **more):
        with _knobs(setting, **more):
            out, nf = gm.generate_mappings(rc, mp, True)
            self.stats = _wide_stats()
        self.arrays = tuple(x.copy() for x in out.arrays())
        self.lf, self.lb, self.nf = out.read_logp()[1].copy(), out.read_logp_backward()[1].copy(), nf.copy()

    def same_bits(self, other):
        return (all(np.array_equal(a, b) for a, b in zip(self.arrays, other.arrays)) and np.array_equal(self.lf, other.lf)
                and np.array_equal(self.lb, other.lb) and np.array_equal(self.nf, other.nf))


def _oracle_sums(oracle, arrays, reads, rc, arr):
    """sum over the reads of the oracle's run_with_mapping(read, its lists).to_edge_and_init_freqs() -> (lf, ef, inf)"""
    om = oracle.Model(arrays)
    off = rc.offsets.astype(np.int64)
    lf, ef, inf = np.zeros(len(reads)), np.zeros(arrays.n_edges), np.zeros(arrays.n_nodes)
    for i, r in enumerate(reads):
        o = om.run_with_mapping(r, oracle.Mapping(*subset_csr(off, arr, [i])))
        lf[i] = o.to_full_prob_forward()
        e1, n1 = o.to_edge_and_init_freqs()
        ef += e1
        inf += n1
    return lf, ef, inf


def _hold_to_oracle(what, run, want, n_reads):
    d = run.dev(*want)
    print(f"{what}: max |d ln P| {d[0]:.3e}, |d edge freq| {d[1]:.3e}, |d init freq| {d[2]:.3e} (bound {TOL_FREQ * n_reads:.1e})")
    assert max(d) <= TOL_FREQ * n_reads


def _kernels_agree(what, a, b, n_reads):
    d = a.dev(b.lf, b.ef, b.inf)
    print(f"{what}: max |d ln P| {d[0]:.3e}, |d edge freq| {d[1]:.3e}, |d init freq| {d[2]:.3e}")
    assert d[0] <= TOL_LOGP and max(d[1:]) <= TOL_FREQ * n_reads


# ------------------------------------------------------------------ crafted lists: boundary widths
def pad_lists(po, nd, reads, n_nodes, seed=5):
    """the list of read j at two of every three positions padded with distinct other nodes, in shuffled order, to width
    WIDTHS[j % 8]; every third position keeps its own short list -> (pos_off, nodes)"""
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
def crafted(oracle):
    arrays, sg = small_dbg_model(600, 12, 0.01, seed=3)
    reads = D.sample_reads(arrays, 10 ** 9, 120, seed=4, max_reads=24)
    assert arrays.n_nodes == 740 and len(reads) == 24
    (po, nd, lp), _ = oracle.Model(arrays).generate_mappings(reads, None, True, n_threads=8)
    ppo, pnd = pad_lists(po, nd, reads, arrays.n_nodes)
    lists = (ppo, pnd, np.zeros(pnd.size))
    rc = D.ReadCollection(reads)
    # the oracle alone accepts these inputs
    want = _oracle_sums(oracle, arrays, reads, rc, lists)
    assert all(np.all(np.isfinite(x)) for x in want)
    return arrays, sg, reads, lists, want, nd


@pytest.fixture(scope="module")
def crafted_runs(gpu_lib, crafted):
    """the call of case 1, the same call with the backward half and then both halves on the generic kernels"""
    arrays, sg, reads, (ppo, pnd, _), want, _ = crafted
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    mp = D.Mappings.from_arrays(rc, ppo, pnd)
    return gm, rc, mp, _Edges(gm, rc, mp, BOTH), _Edges(gm, rc, mp, FWD_ONLY), _Edges(gm, rc, mp, GENERIC)


def test_boundary_widths(crafted, crafted_runs):
    """Fails without the feature: the edges call reports its forward's entries only."""
    arrays, sg, reads, (ppo, pnd, _), want, _ = crafted
    gm, rc, mp, block, fwd_only, generic = crafted_runs
    rmax = _read_max(rc, ppo)
    assert sorted(set(rmax.tolist())) == sorted(WIDTHS)
    _hold_to_oracle("crafted widths", block, want, len(reads))
    launches, cells = block.stats
    wide = _entries(rc, ppo, rmax > 64)
    print(f"crafted widths: wide launches {launches}, cells {cells}, list entries of the wide reads {wide}")
    assert launches >= 2  # forward and backward ran on the block
    assert cells == 2 * wide  # the forward's entries, and the backward computed every position of the same reads


def test_each_half_against_the_kernel_it_restates(crafted, crafted_runs):
    arrays, sg, reads, (ppo, pnd, _), want, _ = crafted
    gm, rc, mp, block, fwd_only, generic = crafted_runs
    n = len(reads)
    assert 0 < fwd_only.stats[0] < block.stats[0]
    assert fwd_only.stats[1] == _entries(rc, ppo, _read_max(rc, ppo) > 64)
    assert generic.stats == (0, 0)
    _kernels_agree("block / forward only", block, fwd_only, n)
    _kernels_agree("block / generic", block, generic, n)
    _kernels_agree("forward only / generic", fwd_only, generic, n)
    # lists of at most 64 nodes: the same kernels in all three runs
    short = np.flatnonzero(_read_max(rc, ppo) <= 64)
    assert short.size == 3
    assert np.array_equal(block.lf[short], fwd_only.lf[short]) and np.array_equal(block.lf[short], generic.lf[short])
    # the new knob without the class: the generic kernels, the bits of the NO knob
    alone = _Edges(gm, rc, mp, {"PHMM_WIDE_EDGE_BWD": "1"})
    assert alone.stats == (0, 0) and alone.same_bits(generic)
    # the backward held to the generic kernel: the call of PHMM_WIDE_HINTED alone
    held = _Edges(gm, rc, mp, BOTH, PHMM_NO_WIDE_LIST_BWD="1")
    assert held.stats == fwd_only.stats and held.same_bits(fwd_only)


def test_same_bits_on_a_second_call(crafted_runs):
    """pool offsets and the order of the blocks leave no trace"""
    gm, rc, mp, block, fwd_only, generic = crafted_runs
    again = _Edges(gm, rc, mp, BOTH)
    assert again.stats == block.stats and again.same_bits(block)


# ------------------------------------------------------------------ read ends
def test_read_ends_on_hand_built_lists(gpu_lib, oracle):
    """reads of 1, 2 and 5 bases and a few of 20-70: merged index len, b_init as prev, position 0 with Begin terms only,
    and the Begin terms over b_init at both ends (not 0 on reads this short).  Lists are the oracle's dense posteriors
    cut to a per-read width of 65-130 nodes: every read runs on the block."""
    arrays, _ = small_dbg_model(300, 12, 0.01, seed=5, min_copy_num=1)
    om = oracle.Model(arrays)
    reads = D.sample_reads(arrays, 10 ** 9, 70, seed=11, max_reads=8)
    reads = [reads[0][:1], reads[1][:2], reads[2][:5]] + [r[: 20 + 10 * j] for j, r in enumerate(reads[3:])]
    assert [len(r) for r in reads] == [1, 2, 5, 20, 30, 5, 50, 60]  # (the sixth read is 5 bases long as sampled)
    widths = [65, 130, 128, 129, 66, 100, 127, 90]
    po, nd = [0], []
    for r, w in zip(reads, widths):
        m = om.run(r).to_mapping(w)
        for i in range(len(r)):
            nodes = m.nodes(i)
            nd.extend(nodes)
            po.append(po[-1] + len(nodes))
    rc = D.ReadCollection(reads)
    po, nd = np.array(po, dtype=np.uint64), np.array(nd, dtype=np.uint32)
    assert _read_max(rc, po).tolist() == widths
    mp = D.Mappings.from_arrays(rc, po, nd)
    gm = D.PHMMModel(arrays)
    want = _oracle_sums(oracle, arrays, reads, rc, (po, nd, np.zeros(nd.size)))
    assert np.max(want[2]) > 1e-3
    for t in ("448", "128"):
        run = _Edges(gm, rc, mp, BOTH, PHMM_WIDE_BWD_T=t)
        assert run.stats[1] == 2 * int(po[-1])  # every read, both halves
        _hold_to_oracle(f"read ends, block of {t}", run, want, len(reads))
    _kernels_agree("read ends, block / generic", run, _Edges(gm, rc, mp, GENERIC), len(reads))


# ------------------------------------------------------------------ real wide lists on tandem repeats
@pytest.fixture(scope="module")
def u20(gpu_lib):
    arrays, reads, _, _ = dataset("u20", 40, max_reads=24)
    assert len(reads) == 24
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    with _knobs({}):
        mp, _ = gm.generate_mappings(rc, None, True)
    rmax = _read_max(rc, mp.arrays()[0])
    print(f"u20: longest list per read {int(rmax.min())} .. {int(rmax.max())}, {int(np.sum(rmax <= 128))} of {rmax.size} at most 128")
    assert np.all((rmax > 64) & (rmax <= 256))
    return arrays, reads, gm, rc, mp, rmax


def test_real_wide_lists_u20(oracle, u20):
    arrays, reads, gm, rc, mp, rmax = u20
    run = _Edges(gm, rc, mp, BOTH)
    assert run.stats[0] >= 2 and run.stats[1] == 2 * int(mp.arrays()[0][-1])
    _hold_to_oracle("u20", run, _oracle_sums(oracle, arrays, reads, rc, mp.arrays()), len(reads))


def test_real_wide_lists_u20n200(gpu_lib, oracle):
    arrays, reads, _, _ = dataset("u20n200", 40)
    rng = np.random.default_rng(5)
    reads = [reads[int(i)][:400] for i in rng.choice(len(reads), 3, replace=False)]
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    with _knobs({}):
        mp, _ = gm.generate_mappings(rc, None, True)
    rmax = _read_max(rc, mp.arrays()[0])
    print(f"u20n200: longest list per read {int(rmax.min())} .. {int(rmax.max())}")
    assert np.all((rmax > 256) & (rmax <= 400))
    run = _Edges(gm, rc, mp, BOTH)
    assert run.stats[0] >= 2 and run.stats[1] == 2 * int(mp.arrays()[0][-1])
    _hold_to_oracle("u20n200", run, _oracle_sums(oracle, arrays, reads, rc, mp.arrays()), len(reads))


# ------------------------------------------------------------------ what stays on the generic kernels
def test_degree_above_the_packed_records(gpu_lib):
    """a graph of degree 7: nothing leaves the generic kernels, and the knobs change no bit"""
    arrays = zoo_model(zoo_graph())
    reads = D.sample_reads(arrays, 10 ** 9, 60, seed=2, max_reads=4)
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    with _knobs({}):
        po, nd, _ = gm.generate_mappings(rc, None, True)[0].arrays()
    ppo, pnd = pad_lists(po, nd, reads, arrays.n_nodes)  # (to widths 64, 65, 128, 129 where the own list is shorter)
    assert np.all(_read_max(rc, ppo) >= 64) and np.sum(_read_max(rc, ppo) > 64) >= 3
    mp = D.Mappings.from_arrays(rc, ppo, pnd)
    generic = _Edges(gm, rc, mp, GENERIC)
    for t in ("448", "128"):
        on = _Edges(gm, rc, mp, BOTH, PHMM_WIDE_BWD_T=t)
        assert on.stats == (0, 0) and on.same_bits(generic)


def test_edge_at_copy_number_zero_on_a_listed_path(oracle, crafted):
    """nodes no read needs go to copy number 0 (min_copy_num 0: their edges weigh 0); the padded lists still name them and
    their parents, so the block meets edges whose term is skipped, not stored"""
    arrays, sg, reads, (ppo, pnd, _), _, own = crafted
    spare = np.setdiff1d(np.unique(pnd), np.unique(own))  # listed by the padding alone
    assert spare.size >= 8
    cn = sg.copy_num.copy()
    cn[spare[:8]] = 0
    with np.errstate(divide="ignore"):
        a2 = D.vectorised_to_phmm(D.SeqGraph(cn, sg.base, sg.edge_src, sg.edge_dst, None), arrays.param, 0)
    rc = D.ReadCollection(reads)
    want = _oracle_sums(oracle, a2, reads, rc, (ppo, pnd, np.zeros(pnd.size)))
    assert np.all(np.isfinite(want[0]))  # every read keeps a positive probability
    gm, mp = D.PHMMModel(a2), D.Mappings.from_arrays(rc, ppo, pnd)
    run = _Edges(gm, rc, mp, BOTH)
    assert run.stats[1] == 2 * _entries(rc, ppo, _read_max(rc, ppo) > 64)
    _hold_to_oracle("zero-weight edges", run, want, len(reads))
    zero_edges = np.flatnonzero(np.isin(sg.edge_src, spare[:8]) | np.isin(sg.edge_dst, spare[:8]))
    assert zero_edges.size and np.all(run.ef[zero_edges] == 0.0)


# ------------------------------------------------------------------ refusals are the generic kernels' refusals
def _status(fn):
    try:
        fn()
    except D.PhmmError as e:
        return e.code
    return _ffi.PHMM_OK


@pytest.mark.parametrize("size", ["448", "128"])
def test_refusals_are_unchanged(gpu_lib, crafted, size):
    arrays, sg, reads, (ppo, pnd, _), _, _ = crafted
    gm, rc_all = D.PHMMModel(arrays), D.ReadCollection(reads)
    mp_all = D.Mappings.from_arrays(rc_all, ppo, pnd)
    rc2 = D.ReadCollection(reads[:2])
    n = len(reads[0]) + len(reads[1])
    # every node listed at bases 100..105 of read 7 (lists of 400 nodes) goes to copy number 0: the read is cut there
    p0 = int(rc_all.offsets[7])
    cn = sg.copy_num.copy()
    cn[np.unique(pnd[int(ppo[p0 + 100]):int(ppo[p0 + 106])])] = 0
    with np.errstate(divide="ignore"):
        a2 = D.vectorised_to_phmm(D.SeqGraph(cn, sg.base, sg.edge_src, sg.edge_dst, None), arrays.param, 0)
    cut = D.PHMMModel(a2)

    def list_of_401():  # (refused where the lists are handed over)
        over = D.Mappings.from_arrays(rc2, np.arange(n + 1, dtype=np.uint64) * 401, np.tile(np.arange(401, dtype=np.uint32), n))
        gm.run_with_mapping_edge_freqs(rc2, over)

    got = {}
    for name, setting in (("block", dict(BOTH, PHMM_WIDE_BWD_T=size)), ("generic", GENERIC)):
        with _knobs(setting):
            got[name] = (_status(lambda: gm.run_with_mapping_edge_freqs(rc2, mp_all)), _status(list_of_401),
                         _status(lambda: cut.run_with_mapping_edge_freqs(rc_all, mp_all)))
    assert got["block"] == (_ffi.PHMM_EINVAL, _ffi.PHMM_ECAPACITY, _ffi.PHMM_EINVAL)
    assert got["generic"] == got["block"]


# ------------------------------------------------------------------ the 128-thread size of the list backward
def _sizes_agree(what, gm, rc, mp, rmax):
    """PHMM_WIDE_BWD_T=128 against 448: the same bits from both calls, one more launch where reads of both kinds exist"""
    extra = 1 if np.any((rmax > 64) & (rmax <= 128)) and np.any(rmax > 128) else 0
    for name, kind, setting in (("lists call", _Lists, FWD_ONLY), ("edges call", _Edges, BOTH)):
        big, small = kind(gm, rc, mp, setting, PHMM_WIDE_BWD_T="448"), kind(gm, rc, mp, setting, PHMM_WIDE_BWD_T="128")
        print(f"{what}, {name}: (launches, cells) with 448 forced {big.stats}, with 128 forced {small.stats}")
        assert small.same_bits(big)
        assert small.stats[0] == big.stats[0] + extra and small.stats[1] == big.stats[1]
        # nothing forced: a handful of reads (fewer than 448-thread blocks the device holds at once) stays on one size
        auto = kind(gm, rc, mp, setting)
        assert auto.stats == big.stats and auto.same_bits(big)
    return extra


def test_block_of_128_threads_crafted(crafted, crafted_runs):
    """Fails without the feature: the knob is unknown and the launch counts are equal."""
    arrays, sg, reads, (ppo, pnd, _), want, _ = crafted
    gm, rc, mp, block, fwd_only, generic = crafted_runs
    # (reads of width 65 and 128 take the small block, 129 and up the large one)
    assert _sizes_agree("crafted widths", gm, rc, mp, _read_max(rc, ppo)) == 1
    small = _Edges(gm, rc, mp, BOTH, PHMM_WIDE_BWD_T="128")
    _hold_to_oracle("crafted widths, block of 128", small, want, len(reads))


def test_block_of_128_threads_u20(u20):
    arrays, reads, gm, rc, mp, rmax = u20
    _sizes_agree("u20", gm, rc, mp, rmax)
