"""GPU: state posteriors over mapping lists (phmm_run_with_mapping_states, PHMMModel.run_with_mapping_states):
PHMMModel::run_with_mapping (freq.rs:72-76) of every read on its lists, then per read position p
PHMMOutput::to_emit_probs(p + 1) by state (table.rs:500-505) over the entries of the input lists, and the head of its
to_states() (table.rs:215-254).

Everything goes through the C ABI and is held, entry by entry and state by state, to the oracle's
run_with_mapping(read, its lists).to_emit_probs(p + 1) indexed at the listed nodes.

Bars: an entry whose oracle value is >= ln 1e-12 within 1e-8 (the bar table entries are held to); one below that must be
below ln 1e-12 + 1e-8 on the GPU, -inf allowed (a scaled column cannot hold what lies 700 nats under its maximum).  No
entry is left out.  ln P per read 1e-9.  The best state must equal a numpy restatement of the reference's rule (stable
ascending sort of Match.., Ins.., Del.., reversed, head) applied to the GPU's own values, name a state the oracle puts
within 1e-8 of the position's maximum, and come out the same with out_state_logp = NULL.

Knobs: PHMM_WIDE_HINTED=1 puts the forward half of reads with lists of 65-400 nodes on a block, PHMM_WIDE_STATES_BWD=1
beside it the backward half, PHMM_NO_WIDE_LIST_BWD=1 holds the backward to the generic kernel, PHMM_NO_WIDE_HINTED=1
both halves; PHMM_WIDE_BWD_T=128 / 448 chooses the block's size.  pad_lists and the crafted inputs are those of
test_gpu_edges_wide.py (restated: a test module cannot be imported from another)."""
import math
import os

import numpy as np
import pytest

import dbgphmm_amd as D
from dbgphmm_amd import _ffi
from helpers import small_dbg_model, subset_csr
from repeat_cases import dataset

pytestmark = pytest.mark.gpu
WIDTHS = (64, 65, 128, 129, 256, 257, 399, 400)
STATS_WIDE = 4
LN_FLOOR = math.log(1e-12)
TOL = 1e-8       # state values at or above the floor
TOL_LOGP = 1e-9  # ln P per read
TOL_SUM = 1e-9   # logsumexp of an entry's three states against the list value of generate_mappings
NONE = 0xFFFFFFFF
KNOBS = ("PHMM_WIDE_HINTED", "PHMM_NO_WIDE_HINTED", "PHMM_WIDE_STATES_BWD", "PHMM_WIDE_EDGE_BWD", "PHMM_NO_WIDE_LIST_BWD",
         "PHMM_WIDE_BWD_T")
BOTH = {"PHMM_WIDE_HINTED": "1", "PHMM_WIDE_STATES_BWD": "1"}
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


def numpy_best(po, sl):
    """the head of to_states() per position from the values themselves: Match.., Ins.., Del.. in slot order, a stable
    ascending sort, reversed (table.rs:228-238) -> (slot << 2) | kind, NONE where nothing is finite"""
    po = po.astype(np.int64)
    out = np.full(po.size - 1, NONE, dtype=np.uint32)
    for g in range(po.size - 1):
        n = int(po[g + 1] - po[g])
        if n == 0:
            continue
        flat = sl[po[g]:po[g + 1]].T.reshape(-1)  # kind-major
        head = int(np.argsort(flat, kind="stable")[::-1][0])
        if flat[head] > -np.inf:
            out[g] = ((head % n) << 2) | (head // n)
    return out


class _States:
    """what one run_with_mapping_states(rc, mp) call returned, the best states of a second call without the values, and
    index 4 of the first call's statistics"""

    def __init__(self, gm, rc, mp, setting, **more):
        with _knobs(setting, **more):
            lf, sl, best = gm.run_with_mapping_states(rc, mp)
            self.stats = _wide_stats()
            _, none, best_only = gm.run_with_mapping_states(rc, mp, want_states=False)
        assert none is None
        self.lf, self.sl, self.best, self.best_only = lf.copy(), sl.copy(), best.copy(), best_only.copy()

    def same_bits(self, other):
        return (np.array_equal(self.lf, other.lf) and np.array_equal(self.sl, other.sl) and np.array_equal(self.best, other.best)
                and np.array_equal(self.best_only, other.best_only))


def oracle_states(oracle, arrays, reads, rc, arr):
    """the oracle's run_with_mapping(read, its lists).to_emit_probs(p + 1) at the listed nodes -> (lf[R], want[entries, 3])"""
    om = oracle.Model(arrays)
    off = rc.offsets.astype(np.int64)
    po, nd = arr[0].astype(np.int64), arr[1]
    want = np.full((int(po[-1]), 3), np.nan)
    lf = np.zeros(len(reads))
    for i, r in enumerate(reads):
        o = om.run_with_mapping(r, oracle.Mapping(*subset_csr(off, (arr[0], arr[1], np.zeros(arr[1].size)), [i])))
        lf[i] = o.to_full_prob_forward()
        for p in range(len(r)):
            a0, a1 = int(po[off[i] + p]), int(po[off[i] + p + 1])
            m, ins, d, _ = o.to_emit_probs(p + 1)
            v = nd[a0:a1]
            want[a0:a1, 0], want[a0:a1, 1], want[a0:a1, 2] = m[v], ins[v], d[v]
    assert not np.any(np.isnan(want))
    return lf, want


def _hold_values(what, got, ref):
    """the bars of the module docstring, entry by entry; ref: the oracle's values (or another kernel's)"""
    assert got.shape == ref.shape
    hi = ref >= LN_FLOOR
    with np.errstate(invalid="ignore"):
        d = float(np.max(np.abs(got[hi] - ref[hi]))) if np.any(hi) else 0.0
    low_max = float(np.max(got[~hi])) if np.any(~hi) else -np.inf
    print(f"{what}: {int(hi.sum())} values >= ln 1e-12, max |d| {d:.3e} (bound {TOL:.0e}); {int((~hi).sum())} below, largest on the "
          f"GPU {low_max:.3f} (bound {LN_FLOOR + TOL:.3f})")
    assert not np.any(np.isnan(got))
    assert d <= TOL
    assert low_max < LN_FLOOR + TOL


def _hold_best(what, run, po, want):
    po = po.astype(np.int64)
    assert run.best.shape == (po.size - 1,)
    assert np.array_equal(run.best, numpy_best(po, run.sl)), what + ": best state is not the head of the GPU's own values"
    assert np.array_equal(run.best_only, run.best), what + ": best state differs without out_state_logp"
    worst = 0.0
    for g in range(po.size - 1):
        w = want[po[g]:po[g + 1]]
        top = w.max() if w.size else -np.inf
        if run.best[g] == NONE:
            assert top < LN_FLOOR + TOL, (what, g)
            continue
        slot, kind = int(run.best[g] >> 2), int(run.best[g] & 3)
        assert kind < 3 and slot < w.shape[0]
        worst = max(worst, top - w[slot, kind])
    print(f"{what}: the oracle's value at the GPU's best state is at most {worst:.3e} under the position's maximum")
    assert worst <= TOL


def _hold_to_oracle(what, run, po, want_lf, want):
    d = float(np.max(np.abs(run.lf - want_lf)))
    print(f"{what}: max |d ln P| {d:.3e} (bound {TOL_LOGP:.0e})")
    assert d <= TOL_LOGP
    _hold_values(what, run.sl, want)
    _hold_best(what, run, po, want)


def _kernels_agree(what, a, b):
    assert float(np.max(np.abs(a.lf - b.lf))) <= TOL_LOGP
    _hold_values(what, a.sl, b.sl)
    _hold_values(what + " (reversed)", b.sl, a.sl)


# ------------------------------------------------------------------ 1. every node listed: to_states() of the dense run
def _all_nodes(rc, n_nodes):
    T = int(rc.offsets[-1])
    return D.Mappings.from_arrays(rc, np.arange(T + 1, dtype=np.uint64) * n_nodes, np.tile(np.arange(n_nodes), T))


@pytest.mark.parametrize("which", ["zero_error", "default"])
def test_every_node_listed_is_the_dense_run(gpu_lib, oracle, which):
    """Fails without the feature: the call does not exist."""
    param, read = ((D.PHMMParams.zero_error(), b"CGATC") if which == "zero_error" else (D.PHMMParams.default(), b"ATTCGTCGT"))
    arrays = D.mock_linear().to_phmm(param)
    gm, rc = D.PHMMModel(arrays), D.ReadCollection([read])
    mp = _all_nodes(rc, arrays.n_nodes)
    po, nd, _ = mp.arrays()
    with np.errstate(divide="ignore"):
        want_lf, want = oracle_states(oracle, arrays, [read], rc, (po, nd))
        run = _States(gm, rc, mp, {})
        _hold_to_oracle(f"linear, {which}", run, po, want_lf, want)
        # PHMMOutput.to_emit_probs of the dense run: every node listed, the same product
        out = gm.run(read)
        dense = np.stack([np.stack(out.to_emit_probs(p + 1), axis=1) for p in range(len(read))]).reshape(-1, 3)
    _hold_values(f"linear, {which}, against the dense run", run.sl, dense)
    if which == "zero_error":
        nodes, kinds = (run.best >> 2).astype(np.int64), run.best & 3  # (slot = node: every node listed in order)
        assert np.all(kinds == 0)
        assert bytes(arrays.emission[nodes].tolist()) == read
        edges = set(zip(arrays.edge_src.tolist(), arrays.edge_dst.tolist()))
        assert all((int(a), int(b)) in edges for a, b in zip(nodes[:-1], nodes[1:]))


# ------------------------------------------------------------------ 2. generated lists, one-wave class
@pytest.mark.parametrize("n_reads", [1, 5, 70])
def test_generated_lists_match_oracle(gpu_lib, oracle, n_reads):
    arrays, _ = small_dbg_model(300, 12, 0.01, seed=5)
    reads = D.sample_reads(arrays, 10 ** 9, 60, seed=n_reads, max_reads=n_reads)
    reads = [r[: max(1, len(r) - (j * 7) % 31)] for j, r in enumerate(reads)]
    rc = D.ReadCollection(reads)
    gm = D.PHMMModel(arrays)
    mp, _ = gm.generate_mappings(rc, None, True)
    po, nd, _ = mp.arrays()
    print(f"generated lists, {n_reads} reads: longest list {int(np.max(np.diff(po.astype(np.int64))))}")
    want_lf, want = oracle_states(oracle, arrays, reads, rc, (po, nd))
    run = _States(gm, rc, mp, {})
    _hold_to_oracle(f"generated lists, {n_reads} reads", run, po, want_lf, want)
    # the same posterior, summed: the list values generate_mappings returns on these lists, for the entries it keeps
    kept, _ = gm.generate_mappings(rc, mp, True)
    kpo, knd, klp = kept.arrays()
    po, kpo = po.astype(np.int64), kpo.astype(np.int64)
    with np.errstate(divide="ignore"):
        mx = run.sl.max(axis=1)
        tot = np.where(mx > -np.inf, mx + np.log(np.sum(np.exp(run.sl - np.where(mx > -np.inf, mx, 0.0)[:, None]), axis=1)), -np.inf)
    worst, n = 0.0, 0
    for g in range(po.size - 1):
        slot_of = {int(v): int(po[g]) + s for s, v in enumerate(nd[po[g]:po[g + 1]])}
        for a in range(kpo[g], kpo[g + 1]):
            worst = max(worst, abs(tot[slot_of[int(knd[a])]] - klp[a]))
            n += 1
    print(f"generated lists, {n_reads} reads: {n} kept entries, max |logsumexp of the states - list value| {worst:.3e}")
    assert n > 0 and worst <= TOL_SUM


# ------------------------------------------------------------------ 3. crafted lists: boundary widths
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
    rc = D.ReadCollection(reads)
    # the oracle alone accepts these inputs: ln P and every position's largest value are finite
    want_lf, want = oracle_states(oracle, arrays, reads, rc, (ppo, pnd))
    assert np.all(np.isfinite(want_lf))
    assert np.all(np.isfinite(np.maximum.reduceat(want.max(axis=1), ppo[:-1].astype(np.int64))))
    return arrays, sg, reads, (ppo, pnd), (want_lf, want)


@pytest.fixture(scope="module")
def crafted_runs(gpu_lib, crafted):
    arrays, sg, reads, (ppo, pnd), _ = crafted
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    mp = D.Mappings.from_arrays(rc, ppo, pnd)
    return gm, rc, mp, _States(gm, rc, mp, GENERIC), _States(gm, rc, mp, FWD_ONLY), _States(gm, rc, mp, BOTH)


def test_boundary_widths(crafted, crafted_runs):
    arrays, sg, reads, (ppo, pnd), (want_lf, want) = crafted
    gm, rc, mp, generic, fwd_only, block = crafted_runs
    rmax = _read_max(rc, ppo)
    assert sorted(set(rmax.tolist())) == sorted(WIDTHS)
    for name, run in (("generic", generic), ("forward on the block", fwd_only), ("both halves on the block", block)):
        _hold_to_oracle("crafted widths, " + name, run, ppo, want_lf, want)
    _kernels_agree("block / forward only", block, fwd_only)
    _kernels_agree("block / generic", block, generic)
    _kernels_agree("forward only / generic", fwd_only, generic)
    wide = _entries(rc, ppo, rmax > 64)
    print(f"crafted widths: (launches, cells) generic {generic.stats}, forward only {fwd_only.stats}, both {block.stats}; "
          f"list entries of the wide reads {wide}")
    assert generic.stats == (0, 0)
    assert fwd_only.stats[0] >= 1 and fwd_only.stats[1] == wide
    assert block.stats[0] > fwd_only.stats[0] and block.stats[1] == 2 * wide
    # the new knob without the class: the generic kernels, the bits of the NO knob
    alone = _States(gm, rc, mp, {"PHMM_WIDE_STATES_BWD": "1"})
    assert alone.stats == (0, 0) and alone.same_bits(generic)
    # the backward held to the generic kernel: the call of PHMM_WIDE_HINTED alone
    held = _States(gm, rc, mp, BOTH, PHMM_NO_WIDE_LIST_BWD="1")
    assert held.stats == fwd_only.stats and held.same_bits(fwd_only)
    # PHMM_NO_WIDE_HINTED wins over everything
    off = _States(gm, rc, mp, BOTH, PHMM_NO_WIDE_HINTED="1")
    assert off.stats == (0, 0) and off.same_bits(generic)


def test_same_bits_on_a_second_call(crafted_runs):
    gm, rc, mp, generic, fwd_only, block = crafted_runs
    for setting, first in ((BOTH, block), (GENERIC, generic)):
        again = _States(gm, rc, mp, setting)
        assert again.stats == first.stats and again.same_bits(first)


def test_the_edges_call_is_untouched(crafted_runs):
    gm, rc, mp, generic, fwd_only, block = crafted_runs
    for setting in ({}, {"PHMM_WIDE_HINTED": "1", "PHMM_WIDE_EDGE_BWD": "1", "PHMM_WIDE_STATES_BWD": "1"}):
        with _knobs(setting):
            before = [x.copy() for x in gm.run_with_mapping_edge_freqs(rc, mp)]
            gm.run_with_mapping_states(rc, mp)
            after = gm.run_with_mapping_edge_freqs(rc, mp)
        assert all(np.array_equal(a, b) for a, b in zip(before, after))


# ------------------------------------------------------------------ 4. read ends
def test_read_ends_on_hand_built_lists(gpu_lib, oracle):
    """reads of 1, 2 and 5 bases and a few of 20-60: merged index len against b_init, position len-1 of a one-base read.
    Lists are the oracle's dense posteriors cut to a per-read width of 65-130 nodes: every read can run on the block."""
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
    want_lf, want = oracle_states(oracle, arrays, reads, rc, (po, nd))
    generic = _States(gm, rc, mp, GENERIC)
    assert generic.stats == (0, 0)
    _hold_to_oracle("read ends, generic", generic, po, want_lf, want)
    runs = {}
    for t in ("448", "128"):
        runs[t] = _States(gm, rc, mp, BOTH, PHMM_WIDE_BWD_T=t)
        assert runs[t].stats[1] == 2 * int(po[-1])  # every read, both halves
        _hold_to_oracle(f"read ends, block of {t}", runs[t], po, want_lf, want)
        _kernels_agree(f"read ends, block of {t} / generic", runs[t], generic)
    assert runs["128"].same_bits(runs["448"])
    # the last position of every read is merged index len: F.tables[len-1] against b_init, nothing is -inf by B
    off = rc.offsets.astype(np.int64)
    for i in range(len(reads)):
        a0, a1 = int(po[off[i + 1] - 1]), int(po[off[i + 1]])
        assert np.isfinite(generic.sl[a0:a1]).sum() == np.isfinite(want[a0:a1]).sum() > 0


# ------------------------------------------------------------------ 5. real wide lists on tandem repeats
def _real(oracle, what, arrays, reads, lo, hi):
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    with _knobs({}):
        mp, _ = gm.generate_mappings(rc, None, True)
    po, nd, _ = mp.arrays()
    rmax = _read_max(rc, po)
    print(f"{what}: longest list per read {int(rmax.min())} .. {int(rmax.max())}, {int(np.sum(rmax <= 128))} of {rmax.size} at most 128")
    assert np.all((rmax > lo) & (rmax <= hi))
    want_lf, want = oracle_states(oracle, arrays, reads, rc, (po, nd))
    big = _States(gm, rc, mp, BOTH, PHMM_WIDE_BWD_T="448")
    assert big.stats[0] >= 2 and big.stats[1] == 2 * int(po[-1])
    _hold_to_oracle(what + ", both halves on the block", big, po, want_lf, want)
    small = _States(gm, rc, mp, BOTH, PHMM_WIDE_BWD_T="128")
    extra = 1 if np.any(rmax <= 128) and np.any(rmax > 128) else 0
    print(f"{what}: (launches, cells) with 448 forced {big.stats}, with 128 forced {small.stats}")
    assert small.same_bits(big)
    assert small.stats[0] == big.stats[0] + extra and small.stats[1] == big.stats[1]


def test_real_wide_lists_u20(gpu_lib, oracle):
    arrays, reads, _, _ = dataset("u20", 40, max_reads=24)
    assert len(reads) == 24
    _real(oracle, "u20", arrays, reads, 64, 256)


def test_real_wide_lists_u20n200(gpu_lib, oracle):
    arrays, reads, _, _ = dataset("u20n200", 40)
    rng = np.random.default_rng(5)
    reads = [reads[int(i)][:400] for i in rng.choice(len(reads), 3, replace=False)]
    _real(oracle, "u20n200", arrays, reads, 256, 400)


# ------------------------------------------------------------------ 6. a node that leaves the list
@pytest.mark.parametrize("setting", [GENERIC, BOTH], ids=["generic", "block"])
def test_a_node_that_leaves_the_list(gpu_lib, oracle, setting):
    """every other position p < len-1 of every read gets, at the head of its list, a node that list p+1 does not hold:
    B.tables[p+1] has no element there, the product keeps the forward's element with value 0 (table.rs:320-331)"""
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
        # (the first read's lists are widened to 70 nodes at every third position: it runs in the block class)
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
                gone.append(new_off[-1])
                lst = np.concatenate([[rng.choice(pool)], lst]).astype(np.uint32)
            new.append(lst)
            new_off.append(new_off[-1] + lst.size)
    npo, nnd = np.array(new_off, np.uint64), np.concatenate(new).astype(np.uint32)
    gone = np.array(gone)
    mp = D.Mappings.from_arrays(rc, npo, nnd)
    with np.errstate(divide="ignore"):
        want_lf, want = oracle_states(oracle, arrays, reads, rc, (npo, nnd))
    assert np.all(np.isfinite(want_lf))
    run = _States(gm, rc, mp, setting)
    if setting is BOTH:
        assert run.stats[1] == 2 * _entries(rc, npo, _read_max(rc, npo) > 64) > 0
    _hold_to_oracle("a node leaves the list", run, npo, want_lf, want)
    assert gone.size > 100
    assert np.all(want[gone] == -np.inf) and np.all(run.sl[gone] == -np.inf)
    # the best state never names such an entry (slot 0 of its position) while another one is finite
    pos_of = np.searchsorted(npo.astype(np.int64), gone, side="right") - 1
    assert np.all(npo[pos_of].astype(np.int64) == gone)
    assert np.all(run.best[pos_of] != NONE) and np.all((run.best[pos_of] >> 2) != 0)


# ------------------------------------------------------------------ 7. refusals are those of the edges call
def _status(fn):
    try:
        fn()
    except D.PhmmError as e:
        return e.code
    return _ffi.PHMM_OK


class _Prefilled:
    """outputs of a raw call, pre-filled: a refusal leaves them as they are"""

    def __init__(self, rc, entries):
        self.lf, self.sl = np.full(len(rc), 7.5), np.full((max(entries, 1), 3), 7.5)
        self.best = np.full(rc.total_bases(), 77, dtype=np.uint32)

    def call(self, gm, rc, mp):
        P = lambda a: a.ctypes.data_as(_ffi.C.c_void_p)
        _ffi.check(_ffi.lib().phmm_run_with_mapping_states(gm._h, rc._h, mp._h, P(self.lf), P(self.sl), P(self.best)))

    def untouched(self):
        return bool(np.all(self.lf == 7.5) and np.all(self.sl == 7.5) and np.all(self.best == 77))


@pytest.mark.parametrize("size", ["448", "128"])
def test_refusals_are_those_of_the_edges_call(gpu_lib, crafted, size):
    arrays, sg, reads, (ppo, pnd), _ = crafted
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

    def list_of_401(call):  # (refused where the lists are handed over)
        over = D.Mappings.from_arrays(rc2, np.arange(n + 1, dtype=np.uint64) * 401, np.tile(np.arange(401, dtype=np.uint32), n))
        call(gm, rc2, over)

    got = {}
    for name, setting in (("block", dict(BOTH, PHMM_WIDE_EDGE_BWD="1", PHMM_WIDE_BWD_T=size)), ("generic", GENERIC)):
        with _knobs(setting):
            outs = [_Prefilled(rc2, int(ppo[-1])), _Prefilled(rc2, 401 * n), _Prefilled(rc_all, int(ppo[-1]))]
            got[name] = (_status(lambda: outs[0].call(gm, rc2, mp_all)), _status(lambda: list_of_401(outs[1].call)),
                         _status(lambda: outs[2].call(cut, rc_all, mp_all)))
            assert all(o.untouched() for o in outs)
            edges = lambda m, rc, mp: m.run_with_mapping_edge_freqs(rc, mp)
            assert got[name] == (_status(lambda: edges(gm, rc2, mp_all)), _status(lambda: list_of_401(edges)),
                                 _status(lambda: edges(cut, rc_all, mp_all)))
    assert got["block"] == (_ffi.PHMM_EINVAL, _ffi.PHMM_ECAPACITY, _ffi.PHMM_EINVAL)
    assert got["generic"] == got["block"]


# ------------------------------------------------------------------ output forms
class _DeviceArray:
    """bytes in device memory (the HIP runtime the library is linked against)"""

    def __init__(self, nbytes, fill):
        import ctypes as C
        self.C, self.hip, self.nbytes = C, C.CDLL("libamdhip64.so"), nbytes
        self.p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.p), C.c_size_t(max(nbytes, 1))) == 0
        assert self.hip.hipMemset(self.p, C.c_int(fill), C.c_size_t(max(nbytes, 1))) == 0

    def numpy(self, dtype):
        out = np.empty(self.nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        assert self.hip.hipMemcpy(out.ctypes.data_as(self.C.c_void_p), self.p, self.C.c_size_t(self.nbytes), 2) == 0
        return out

    def __del__(self):
        self.hip.hipFree(self.p)


def test_output_forms(gpu_lib):
    """device-pointer outputs equal host outputs, every output may be NULL, and a call without reads writes nothing"""
    arrays, _ = small_dbg_model(300, 12, 0.01, seed=5, min_copy_num=1)
    reads = D.sample_reads(arrays, 10 ** 9, 60, seed=3, max_reads=20)
    rc = D.ReadCollection(reads)
    gm = D.PHMMModel(arrays)
    with _knobs({}):
        mp, _ = gm.generate_mappings(rc, None, True)
        te = int(mp.arrays()[0][-1])
        lf, sl, best = gm.run_with_mapping_states(rc, mp)
        L = _ffi.lib()
        dl, ds, db = _DeviceArray(8 * len(reads), 0), _DeviceArray(24 * te, 0), _DeviceArray(4 * rc.total_bases(), 0)
        _ffi.check(L.phmm_run_with_mapping_states(gm._h, rc._h, mp._h, dl.p, ds.p, db.p))
        assert np.array_equal(dl.numpy(np.float64), lf) and np.array_equal(ds.numpy(np.float64).reshape(-1, 3), sl)
        assert np.array_equal(db.numpy(np.uint32), best)
        # the best states alone into device memory, the values alone into host memory
        db2 = _DeviceArray(4 * rc.total_bases(), 0)
        _ffi.check(L.phmm_run_with_mapping_states(gm._h, rc._h, mp._h, None, None, db2.p))
        assert np.array_equal(db2.numpy(np.uint32), best)
        lf3, sl3, none = gm.run_with_mapping_states(rc, mp, want_best=False)
        assert none is None and np.array_equal(sl3, sl) and np.array_equal(lf3, lf)
        _ffi.check(L.phmm_run_with_mapping_states(gm._h, rc._h, mp._h, None, None, None))
        # no reads: nothing is written
        rc0 = D.ReadCollection([])
        mp0 = D.Mappings.from_arrays(rc0, np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint32))
        out = _Prefilled(rc0, 0)
        out.lf = np.full(1, 7.5)
        out.call(gm, rc0, mp0)
        assert out.untouched()
