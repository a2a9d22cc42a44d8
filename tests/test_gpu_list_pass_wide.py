"""GPU: the list pass (run_with_mapping, freq.rs:72-76 = forward_with_mapping with stored columns + backward_with_mapping)
on a block for reads whose longest mapping list holds 65-400 nodes: the record-storing flavour of hinted_wide_kernel
(hinted_wide_kernel.h) and wide_backward_kernel<true> (wide_bwd_kernel.h), behind phmm_generate_mappings(mappings != NULL)
and phmm_run_with_mapping_edges.

Everything goes through the C ABI and is held to the oracle's run_with_mapping on the same lists.  The class is opt-in
(PHMM_WIDE_HINTED=1, set for every test here); PHMM_NO_WIDE_LIST_BWD=1 keeps the backward half on the generic kernel,
PHMM_NO_WIDE_HINTED=1 both halves.  pad_lists and the crafted inputs are those of test_gpu_hinted_wide.py (restated: a
test module cannot be imported without editing it)."""
import os

import numpy as np
import pytest

import dbgphmm_amd as D
from dbgphmm_amd import _ffi
from graph_cases import zoo_graph, zoo_model
from helpers import compare_mappings, small_dbg_model, subset_csr
from repeat_cases import dataset

pytestmark = pytest.mark.gpu
WIDTHS = (64, 65, 128, 129, 256, 257, 399, 400)
STATS_WIDE = 4
TOL_LOGP = 1e-9   # ln P per read, forward and backward, and list values between the kernels
TOL_FREQ = 1e-9   # edge / init frequencies, times the number of reads (test_gpu_hinted_edges.py)
TOL_USAGE = 1e-8  # node usage, |differences| summed over the nodes
ACCEPTABLE_ERROR_FORWARD_AND_BACKWARD = 0.01  # dbg.rs:44


class _env:
    """an environment knob for the calls inside the block (knobs are read when a call takes the device)"""

    def __init__(self, name, value="1"):
        self.name, self.value = name, value

    def __enter__(self):
        self.before = os.environ.get(self.name)
        os.environ[self.name] = self.value

    def __exit__(self, *a):
        if self.before is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = self.before


@pytest.fixture(autouse=True)
def _wide_class_on():
    """the class is opt-in; PHMM_NO_WIDE_HINTED inside a test still wins over it"""
    with _env("PHMM_WIDE_HINTED"):
        yield


def _wide_stats():
    ms, launches, cells = _ffi.last_call_stats(STATS_WIDE)
    return launches, cells


def _read_max(rc, po):
    off, cnt = rc.offsets.astype(np.int64), np.diff(po.astype(np.int64))
    return np.array([cnt[off[r]:off[r + 1]].max() if off[r + 1] > off[r] else 0 for r in range(len(rc))])


def _entries(rc, po, which):
    off = rc.offsets.astype(np.int64)
    return int(sum(int(po[off[r + 1]]) - int(po[off[r]]) for r in np.flatnonzero(which)))


class _Run:
    """what one generate_mappings(rc, mp, use_max_ratio) call returned, and index 4 of its statistics"""

    def __init__(self, gm, rc, mp, use_max_ratio=True):
        out, nf = gm.generate_mappings(rc, mp, use_max_ratio)
        self.stats = _wide_stats()
        self.arrays = tuple(x.copy() for x in out.arrays())
        self.lf, self.lb, self.nf = out.read_logp()[1].copy(), out.read_logp_backward()[1].copy(), nf.copy()

    def same_bits(self, other, reads=None, off=None):
        if reads is None:
            return (all(np.array_equal(a, b) for a, b in zip(self.arrays, other.arrays)) and np.array_equal(self.lf, other.lf)
                    and np.array_equal(self.lb, other.lb) and np.array_equal(self.nf, other.nf))
        a, b = subset_csr(off, self.arrays, reads), subset_csr(off, other.arrays, reads)
        return (all(np.array_equal(x, y) for x, y in zip(a, b)) and np.array_equal(self.lf[reads], other.lf[reads])
                and np.array_equal(self.lb[reads], other.lb[reads]))


def _oracle_run(oracle, arrays, reads, lists, use_max_ratio=True):
    """the oracle's run_with_mapping of every read on `lists` -> (mapping arrays, node usage, ln P forward, backward)"""
    om = oracle.Model(arrays)
    out, nf = om.generate_mappings(reads, lists, use_max_ratio, n_threads=8)
    lf = om.full_prob_reads(reads, lists, True, n_threads=8)
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])])
    lb = np.array([om.run_with_mapping(r, oracle.Mapping(*subset_csr(off, lists, [i]))).to_full_prob_backward()
                   for i, r in enumerate(reads)])
    return out, nf, lf, lb


def _usage_per_read(reads, arrays, n_nodes):
    """Mappings::to_node_freqs (hint.rs:161-171) read by read: the sum of a node's list probabilities -> [reads][nodes]"""
    po, nd, lp = arrays
    out = np.zeros((len(reads), n_nodes))
    g = 0
    for i, r in enumerate(reads):
        e0, e1 = int(po[g]), int(po[g + len(r)])
        np.add.at(out[i], nd[e0:e1], np.exp(lp[e0:e1]))
        g += len(r)
    return out


def _hold_to_oracle(what, run, reads, want, per_read=False, **kw):
    """ln P forward and backward within 1e-9 per read, the lists through compare_mappings, node usage within 1e-8 summed
    over the nodes: of the call, or (per_read: real read sets of ~1000 bases, where the rounding of a read's ln P -- some
    1e-13 on values near -100, far inside the bar above -- scales every one of its positions the same way, and 24 000
    positions add that up past 1e-8 for the generic kernels and the block alike) of each read, from its lists"""
    out, nf, lf, lb = want
    d_lf, d_lb = float(np.max(np.abs(run.lf - lf))), float(np.max(np.abs(run.lb - lb)))
    d_nf = float(np.abs(run.nf - nf).sum())
    if per_read:
        mine, theirs = _usage_per_read(reads, run.arrays, nf.size), _usage_per_read(reads, out, nf.size)
        d_call, d_nf = d_nf, float(np.abs(mine - theirs).sum(axis=1).max())
        print(f"{what}: node usage of the whole call, sum |d| {d_call:.3e}")
    print(f"{what}: max |d ln P| forward {d_lf:.3e} backward {d_lb:.3e}, "
          f"node usage sum |d| {d_nf:.3e}{' (largest of a read)' if per_read else ''}")
    compare_mappings(reads, run.arrays, out, **kw)
    assert d_lf <= TOL_LOGP and d_lb <= TOL_LOGP and d_nf <= TOL_USAGE


def _kernels_agree(a, b, ratio):
    """two runs on the same reads and lists by different kernels: list values within 1e-9 in the log, membership
    equal except for entries within 1e-9 of the ratio cut (either side) -> positions with such an entry"""
    (pa, na, la), (pb, nb, lb) = a.arrays, b.arrays
    assert pa.shape == pb.shape
    edge = 0
    for g in range(pa.size - 1):
        x = dict(zip(na[int(pa[g]):int(pa[g + 1])].tolist(), la[int(pa[g]):int(pa[g + 1])].tolist()))
        y = dict(zip(nb[int(pb[g]):int(pb[g + 1])].tolist(), lb[int(pb[g]):int(pb[g + 1])].tolist()))
        assert x and y, g
        for n in set(x) & set(y):
            assert abs(x[n] - y[n]) <= TOL_LOGP, (g, n, x[n], y[n])
        odd = set(x) ^ set(y)
        if odd:
            cut = max(max(x.values()), max(y.values())) - ratio
            assert all(abs((x.get(n, y.get(n))) - cut) <= TOL_LOGP for n in odd), (g, sorted(odd))
            edge += 1
    return edge


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
    # the oracle alone accepts these inputs
    want = _oracle_run(oracle, arrays, reads, lists)
    assert np.all(np.isfinite(want[2])) and np.all(np.isfinite(want[3]))
    assert np.all(np.diff(want[0][0].astype(np.int64)) > 0)
    return arrays, sg, reads, lists, want


@pytest.fixture(scope="module")
def crafted_runs(gpu_lib, crafted):
    """the call of case 1 and the same call with the backward half, then both halves, on the generic kernels"""
    arrays, sg, reads, (ppo, pnd, _), want = crafted
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    mp = D.Mappings.from_arrays(rc, ppo, pnd)
    with _env("PHMM_WIDE_HINTED"):
        block = _Run(gm, rc, mp)
        with _env("PHMM_NO_WIDE_LIST_BWD"):
            fwd_only = _Run(gm, rc, mp)
        with _env("PHMM_NO_WIDE_HINTED"):
            generic = _Run(gm, rc, mp)
    return gm, rc, mp, block, fwd_only, generic


def test_boundary_widths(crafted, crafted_runs):
    """Fails without the feature: a stored-column call reports (0, 0) under index 4."""
    arrays, sg, reads, (ppo, pnd, _), want = crafted
    gm, rc, mp, block, fwd_only, generic = crafted_runs
    rmax = _read_max(rc, ppo)
    assert sorted(set(rmax.tolist())) == sorted(WIDTHS)
    _hold_to_oracle("crafted widths", block, reads, want)
    launches, cells = block.stats
    wide = _entries(rc, ppo, rmax > 64)
    print(f"crafted widths: wide launches {launches}, cells {cells}, list entries of the wide reads {wide}")
    assert launches >= 2  # forward and backward ran on the block
    assert cells == 2 * wide  # the forward's entries, and the backward computed every position of the same reads


def test_each_half_against_the_kernel_it_restates(crafted, crafted_runs):
    arrays, sg, reads, (ppo, pnd, _), want = crafted
    gm, rc, mp, block, fwd_only, generic = crafted_runs
    assert 0 < fwd_only.stats[0] < block.stats[0]
    assert fwd_only.stats[1] == _entries(rc, ppo, _read_max(rc, ppo) > 64)
    assert generic.stats == (0, 0)
    ratio = arrays.param.active_node_max_ratio
    for name, a, b in (("block / forward only", block, fwd_only), ("block / generic", block, generic),
                       ("forward only / generic", fwd_only, generic)):
        d_lf, d_lb = float(np.max(np.abs(a.lf - b.lf))), float(np.max(np.abs(a.lb - b.lb)))
        edge = _kernels_agree(a, b, ratio)
        print(f"{name}: max |d ln P| forward {d_lf:.3e} backward {d_lb:.3e}, positions with an entry at the cut {edge}")
        assert d_lf <= TOL_LOGP and d_lb <= TOL_LOGP
        assert edge <= 1e-4 * (ppo.size - 1)
    # lists of at most 64 nodes: the same kernels in all three runs
    off = rc.offsets.astype(np.int64)
    short = np.flatnonzero(_read_max(rc, ppo) <= 64).tolist()
    assert len(short) == 3
    assert block.same_bits(fwd_only, short, off) and block.same_bits(generic, short, off)
    # not opted in: the generic kernels, the bits of the NO knob
    with _env("PHMM_WIDE_HINTED", "0"):
        plain = _Run(gm, rc, mp)
    assert plain.stats == (0, 0) and plain.same_bits(generic)


def test_same_bits_on_a_second_call_and_on_a_subset(crafted, crafted_runs):
    """pool offsets, the order of the blocks and the reads beside a read leave no trace in its bits"""
    arrays, sg, reads, lists, want = crafted
    gm, rc, mp, block, fwd_only, generic = crafted_runs
    assert _Run(gm, rc, mp).same_bits(block)
    pick = list(range(0, len(reads), 2))
    off = rc.offsets.astype(np.int64)
    rc2 = D.ReadCollection([reads[i] for i in pick])
    po2, nd2, _ = subset_csr(off, lists, pick)
    half = _Run(gm, rc2, D.Mappings.from_arrays(rc2, po2, nd2))
    assert half.stats[0] >= 2
    got = subset_csr(off, block.arrays, pick)
    assert all(np.array_equal(x, y) for x, y in zip(half.arrays, got))
    assert np.array_equal(half.lf, block.lf[pick]) and np.array_equal(half.lb, block.lb[pick])


def test_top_k_keeps_the_generic_backward(oracle, crafted, crafted_runs):
    arrays, sg, reads, lists, want = crafted
    gm, rc, mp, block, fwd_only, generic = crafted_runs
    top = _Run(gm, rc, mp, use_max_ratio=False)
    assert top.stats == fwd_only.stats  # the forward only
    out, _ = oracle.Model(arrays).generate_mappings(reads, lists, False, n_threads=8)
    compare_mappings(reads, top.arrays, out, top_k=arrays.param.n_active_nodes)
    assert np.max(np.abs(top.lf - want[2])) <= TOL_LOGP and np.max(np.abs(top.lb - want[3])) <= TOL_LOGP


def test_degree_above_the_packed_records(gpu_lib):
    """a graph of degree 7: neither half leaves the generic kernels, and the knob changes no bit"""
    arrays = zoo_model(zoo_graph())
    reads = D.sample_reads(arrays, 10 ** 9, 60, seed=2, max_reads=4)
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    po, nd, _ = gm.generate_mappings(rc, None, True)[0].arrays()
    ppo, pnd = pad_lists(po, nd, reads, arrays.n_nodes)  # (to widths 64, 65, 128, 129 where the own list is shorter)
    assert np.all(_read_max(rc, ppo) >= 64) and np.sum(_read_max(rc, ppo) > 64) >= 3
    mp = D.Mappings.from_arrays(rc, ppo, pnd)
    on = _Run(gm, rc, mp)
    assert on.stats == (0, 0)
    with _env("PHMM_NO_WIDE_HINTED"):
        assert _Run(gm, rc, mp).same_bits(on)


# ------------------------------------------------------------------ refusals are the generic kernels' refusals
def _status(fn):
    try:
        fn()
    except D.PhmmError as e:
        return e.code
    return _ffi.PHMM_OK


@pytest.mark.parametrize("knob", ["PHMM_WIDE_HINTED", "PHMM_NO_WIDE_HINTED"])
def test_refusals_are_unchanged(gpu_lib, crafted, knob):
    arrays, sg, reads, (ppo, pnd, _), want = crafted
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads[:2])
    n = len(reads[0]) + len(reads[1])
    with _env(knob):
        for width in (200, 100):  # the 448-thread and the 128-thread block
            lst = np.arange(width, dtype=np.uint32) + 7
            lst[width - 3] = lst[5]
            mp = D.Mappings.from_arrays(rc, np.arange(n + 1, dtype=np.uint64) * width, np.tile(lst, n))
            assert _status(lambda: gm.generate_mappings(rc, mp, True)) == _ffi.PHMM_EINVAL
        def list_of_401():  # (refused where the lists are handed over)
            over = D.Mappings.from_arrays(rc, np.arange(n + 1, dtype=np.uint64) * 401, np.tile(np.arange(401, dtype=np.uint32), n))
            gm.generate_mappings(rc, over, True)
        assert _status(list_of_401) == _ffi.PHMM_ECAPACITY
        # every node listed at bases 100..105 of read 7 (lists of 400 nodes) goes to copy number 0: the read is cut there
        rc_all = D.ReadCollection(reads)
        p0 = int(rc_all.offsets[7])
        cn = sg.copy_num.copy()
        cn[np.unique(pnd[int(ppo[p0 + 100]):int(ppo[p0 + 106])])] = 0
        with np.errstate(divide="ignore"):
            a2 = D.vectorised_to_phmm(D.SeqGraph(cn, sg.base, sg.edge_src, sg.edge_dst, None), arrays.param, 0)
        mp = D.Mappings.from_arrays(rc_all, ppo, pnd)
        assert _status(lambda: D.PHMMModel(a2).generate_mappings(rc_all, mp, True)) == _ffi.PHMM_EINVAL


# ------------------------------------------------------------------ real wide lists on tandem repeats
@pytest.fixture(scope="module")
def n200():
    arrays, reads, _, _ = dataset("u20n200", 40)
    rng = np.random.default_rng(5)
    return arrays, [reads[int(i)][:400] for i in rng.choice(len(reads), 3, replace=False)]


def _real_lists(oracle, arrays, reads, lo, hi):
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    mp, _ = gm.generate_mappings(rc, None, True)
    lists = tuple(x.copy() for x in mp.arrays())
    rmax = _read_max(rc, lists[0])
    print(f"longest list per read: {int(rmax.min())} .. {int(rmax.max())}")
    assert np.all((rmax > lo) & (rmax <= hi))
    run = _Run(gm, rc, mp)
    assert run.stats[0] >= 2 and run.stats[1] == 2 * int(lists[0][-1])
    want = _oracle_run(oracle, arrays, reads, lists)
    with _env("PHMM_NO_WIDE_HINTED"):
        generic = _Run(gm, rc, mp)
    print(f"generic kernels on the same lists: node usage of the whole call, sum |d| {float(np.abs(generic.nf - want[1]).sum()):.3e}")
    _hold_to_oracle("real lists", run, reads, want, per_read=True)  # the oracle per read
    # the reference's own check (dbg.rs:170-172)
    assert np.max(np.abs(run.lf - run.lb)) < ACCEPTABLE_ERROR_FORWARD_AND_BACKWARD


def test_real_wide_lists_u20(gpu_lib, oracle):
    arrays, reads, _, _ = dataset("u20", 40, max_reads=24)
    assert len(reads) == 24
    _real_lists(oracle, arrays, reads, 64, 256)


def test_real_wide_lists_u20n200(gpu_lib, oracle, n200):
    arrays, reads = n200
    _real_lists(oracle, arrays, reads, 256, 400)


def test_edges_call_runs_its_forward_on_the_block(gpu_lib, oracle, n200):
    arrays, reads = n200
    gm, om, rc = D.PHMMModel(arrays), oracle.Model(arrays), D.ReadCollection(reads)
    mp, _ = gm.generate_mappings(rc, None, True)
    lf, ef, inf = gm.run_with_mapping_edge_freqs(rc, mp)
    launches, cells = _wide_stats()
    assert launches > 0 and cells == int(mp.arrays()[0][-1])  # the forward half only
    off = rc.offsets.astype(np.int64)
    olf, oef, oinf = np.zeros(len(reads)), np.zeros(arrays.n_edges), np.zeros(arrays.n_nodes)
    for i, r in enumerate(reads):
        o = om.run_with_mapping(r, oracle.Mapping(*subset_csr(off, mp.arrays(), [i])))
        olf[i] = o.to_full_prob_forward()
        e1, n1 = o.to_edge_and_init_freqs()
        oef += e1
        oinf += n1
    tol = TOL_FREQ * len(reads)
    d = [float(np.max(np.abs(a - b))) for a, b in ((lf, olf), (ef, oef), (inf, oinf))]
    print(f"edges call: max |d ln P| {d[0]:.3e}, |d edge freq| {d[1]:.3e}, |d init freq| {d[2]:.3e}")
    assert max(d) < tol
    lf2, ef2, inf2 = gm.run_with_mapping_edge_freqs(rc, mp)
    assert np.array_equal(lf, lf2) and np.array_equal(ef, ef2) and np.array_equal(inf, inf2)
