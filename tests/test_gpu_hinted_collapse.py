"""GPU: the collapse detector of the hinted forward kernels swept across its threshold.

A candidate that sets every node a read's lists hold at six consecutive bases to copy number 0 cuts the read there:
the reference's ln P stays finite, because the InsBegin chain (p_random p_II per base) re-enters the graph behind the
cut, but it falls with the position of the cut -- here by about 55 + 7.2 c nats for a cut at base c.  The scaled linear
kernels (hinted_score_kernel, hinted_lean_kernel, hinted_packed_kernel, hinted_wide_kernel) cannot follow a column
maximum that falls by more than 2^512 in one position (HINT_COLLAPSE_EXP) and flag such a (candidate, read) pair, as
they do a final sum of zero; flagged pairs are recomputed in log space.  A detector that passes a pair it should have
flagged gives a finite, plausible, wrong ln P.  The suite's other cut reads are cut at bases 200-300, far on the safe
side; here the cut moves one base per candidate from 24 to 124, across the points where the one-position drop reaches
512, 1022 and 1074 bits (c of about 49, 98 and 103).

PHMM_NO_EXACT_HINTED=1 shows what the detector decided: a flagged pair comes back -inf, so every pair that is NOT -inf
has to equal the oracle at the bar of the unflagged path (1e-9)."""
import numpy as np
import pytest

import dbgphmm_amd as D
from helpers import small_dbg_model
from test_gpu_hinted_wide import _env, _host_model, _maxdiff, _oracle_scores, _read_max, _wide_stats, repeat  # noqa: F401
# (repeat: the tandem-repeat fixture of that file)

pytestmark = pytest.mark.gpu
CUTS = tuple(range(24, 125))
CLASSES = ((), ("PHMM_NO_PACKED",), ("PHMM_NO_PACKED", "PHMM_NO_LEAN"))
TOL = 1e-9


class _envs:
    """several knobs set to 1 for the calls inside the block"""

    def __init__(self, *names):
        self.ctx = [_env(n) for n in names]

    def __enter__(self):
        for c in self.ctx:
            c.__enter__()

    def __exit__(self, *a):
        for c in reversed(self.ctx):
            c.__exit__(*a)


def _cut_vector(base, lists, first_pos, c):
    """every node listed at bases c .. c+5 of the read whose lists start at position first_pos -> copy number 0"""
    po, nd, _ = lists
    v = base.copy()
    v[np.unique(nd[int(po[first_pos + c]):int(po[first_pos + c + 6])])] = 0
    return v


class Sweep:
    pass


@pytest.fixture(scope="module")
def sweep(oracle):
    s = Sweep()
    arrays, sg = small_dbg_model(900, 12, 0.003, seed=21, min_copy_num=1)
    assert arrays.n_nodes == 1080
    reads = [r[:260] for r in D.sample_reads(arrays, 10 ** 9, 420, seed=21, max_reads=40) if len(r) > 380][:8]
    assert len(reads) == 8
    s.sg, s.param, s.reads = sg, arrays.param, reads
    s.lists, _ = oracle.Model(arrays).generate_mappings(reads, None, True, n_threads=8)
    s.base = sg.copy_num.astype(np.uint32)
    s.cands = np.array([_cut_vector(s.base, s.lists, 0, c) for c in CUTS], np.uint32)
    s.models = [_host_model(sg, s.param, v, 0) for v in s.cands]
    s.want = np.array([oracle.Model(m).full_prob_reads(reads, s.lists, True, n_threads=8) for m in s.models])
    s.base_lp = _oracle_scores(oracle, sg, s.param, reads, s.lists, s.base, 0)
    assert np.all(np.isfinite(s.want)) and np.all(np.isfinite(s.base_lp))
    # the inputs: read 0's score falls by about 55 + 7.2 c nats, from under 512 bits to over 1074; other reads are cut too
    bits = (s.base_lp[0] - s.want[:, 0]) / np.log(2.0)
    assert bits[0] < 400.0 and bits[-1] > 1200.0 and np.all(np.diff(bits) > 0) and np.max(np.diff(bits)) < 16.0
    assert ((s.base_lp[None, 1:] - s.want[:, 1:]).max(axis=0) > 100.0).sum() >= 3
    return s


def _handles(s):
    gm = D.PHMMModel(_host_model(s.sg, s.param, s.base, 0))
    rc = D.ReadCollection(s.reads)
    return gm, rc, D.Mappings.from_arrays(rc, *s.lists)


def _full_forms(gm, rc, mp, cands, models):
    by_cn = gm.to_full_prob_reads_copy_nums(rc, mp, cands, 0)[1]
    by_prob = gm.to_full_prob_reads_candidates(rc, mp, np.array([m.init_logp for m in models]),
                                               np.array([m.trans_logp for m in models]))[1]
    return (("copy numbers", by_cn), ("probability vectors", by_prob))


def _sound(got, want):
    """-> (every pair that is not -inf is within TOL of the oracle, largest deviation of those pairs)"""
    kept = ~np.isneginf(got)
    with np.errstate(invalid="ignore"):
        dev = np.abs(got - want)[kept]
    return bool(np.all(dev <= TOL)), float(np.max(dev, initial=0.0))  # (a NaN fails the comparison)


@pytest.mark.parametrize("cls", CLASSES, ids=["default", "no_packed", "no_packed_no_lean"])
def test_kept_pairs_equal_the_oracle(gpu_lib, sweep, cls):
    s = sweep
    gm, rc, mp = _handles(s)
    with _envs("PHMM_NO_EXACT_HINTED", *cls):
        forms = _full_forms(gm, rc, mp, s.cands, s.models)
    for name, got in forms:
        ok, dev = _sound(got, s.want)
        lost0 = np.isneginf(got[:, 0])
        first = CUTS[int(np.argmax(lost0))] if lost0.any() else None
        print(f"{'+'.join(cls) or 'default'}, {name}: read 0 first -inf at c = {first}, {int((~lost0).sum())} kept / "
              f"{int(lost0.sum())} -inf; -inf pairs of the other reads {np.isneginf(got[:, 1:]).sum(axis=0).tolist()}; "
              f"kept pairs max |GPU - oracle| {dev:.3e}")
        assert ok, (cls, name, dev)
        assert (~lost0).sum() >= 10 and lost0.sum() >= 10, (cls, name)
    with _envs(*cls):
        forms = _full_forms(gm, rc, mp, s.cands, s.models)
    for name, got in forms:
        print(f"{'+'.join(cls) or 'default'}, {name}, fallback on: max |GPU - oracle| {_maxdiff(got, s.want):.3e}")
        assert np.all(np.isfinite(got)) and _maxdiff(got, s.want) <= TOL, (cls, name)


def _change_tol(s):
    """the bars of the change-form suites: 1e-9, 1e-6 for a read more than 100 nats below its base score"""
    return np.where(s.base_lp[None, :] - s.want > 100.0, 1e-6, 1e-9)


def test_change_forms(gpu_lib, sweep):
    s = sweep
    gm, rc, mp = _handles(s)
    changes = D.copy_num_changes(s.base, s.cands)
    tol = _change_tol(s)
    _, lp_s, n_s = gm.to_full_prob_reads_copy_num_changes(rc, mp, s.base, changes, 0)
    lk = gm.likelihood(rc, mp, s.base, 0)
    _, lp_h, n_h = lk.score_changes(changes)
    assert np.array_equal(n_s, n_h) and np.all(n_s >= 1)
    for name, got in (("stateless change form", lp_s), ("handle score_changes", lp_h)):
        dev = np.abs(got - s.want)
        print(f"{name}: max |GPU - oracle| {dev.max():.3e} (pairs held to 1e-9: {dev[tol < 1e-8].max():.3e})")
        assert np.all(np.isfinite(got)) and np.all(dev <= tol), name


def test_handle_moves(gpu_lib, sweep):
    s = sweep
    gm, rc, mp = _handles(s)
    lk = gm.likelihood(rc, mp, s.base, 0)
    tol = _change_tol(s)
    worst = 0.0
    for c in (44, 52, 100, 108):
        j = CUTS.index(c)
        nodes = np.flatnonzero(s.cands[j] != s.base).astype(np.uint32)
        lk.move(nodes, s.cands[j][nodes])
        cn, cur, _ = lk.current()
        full = gm.to_full_prob_reads_copy_nums(rc, mp, s.cands[j][None, :], 0)[1][0]
        assert np.array_equal(cn, s.cands[j])
        assert np.all(np.isfinite(cur)) and np.max(np.abs(cur - full)) <= TOL, c
        assert np.all(np.abs(cur - s.want[j]) <= tol[j]), c
        lk.refresh()
        cn2, again, _ = lk.current()
        assert np.array_equal(cn2, cn) and np.max(np.abs(again - cur)) <= TOL, c
        assert np.all(np.abs(again - s.want[j]) <= tol[j]), c
        worst = max(worst, float(np.max(np.abs(cur - s.want[j]))), float(np.max(np.abs(again - s.want[j]))))
        lk.move(nodes, s.base[nodes])
        cn3, back, _ = lk.current()
        assert np.array_equal(cn3, s.base) and np.max(np.abs(back - s.base_lp)) <= TOL, c
    print(f"handle moves to c = 44, 52, 100, 108: max |current - oracle| {worst:.3e}")


def test_wide_class(gpu_lib, oracle, repeat):
    """the same sweep, four bases per step, on a read of the tandem repeat whose longest list exceeds 64 nodes"""
    sg, param, reads, lists = repeat
    rc = D.ReadCollection(reads)
    mp = D.Mappings.from_arrays(rc, *lists)
    rmax = _read_max(rc, lists[0])
    r = int(np.flatnonzero((rmax > 64) & (np.array([len(x) for x in reads]) >= 130))[0])
    first_pos = int(rc.offsets[r])
    base = sg.copy_num.astype(np.uint32)
    cuts = tuple(range(24, 125, 4))
    cands = np.array([_cut_vector(base, lists, first_pos, c) for c in cuts], np.uint32)
    models = [_host_model(sg, param, v, 0) for v in cands]
    want = np.array([oracle.Model(m).full_prob_reads(reads, lists, True, n_threads=8) for m in models])
    # The repeat puts every copy of a unit on the lists, so these candidates zero 70-300 nodes and cut read r thousands
    # of bits deep wherever they fall; the other wide reads are cut by the same candidates at other depths.  The inputs
    # must hold wide pairs on both sides: a pair whose ln P is above -400 bits cannot lose 2^512 in one position, one
    # below -1200 bits is past every threshold
    wide = rmax > 64
    neg_bits = -want[:, wide] / np.log(2.0)
    print(f"read {r}, longest list {int(rmax[r])}; wide reads {int(wide.sum())}; -ln P of their pairs: "
          f"{int((neg_bits < 400.0).sum())} under 400 bits, {int((neg_bits > 1200.0).sum())} over 1200 bits, "
          f"{int(((neg_bits >= 400.0) & (neg_bits <= 1200.0)).sum())} between")
    assert np.all(np.isfinite(want)) and (neg_bits < 400.0).sum() >= 10 and (neg_bits > 1200.0).sum() >= 10
    gm = D.PHMMModel(_host_model(sg, param, base, 0))
    with _env("PHMM_WIDE_HINTED"):
        with _env("PHMM_NO_EXACT_HINTED"):
            forms = _full_forms(gm, rc, mp, cands, models)
            assert _wide_stats()[1] > 0
        for name, got in forms:
            ok, dev = _sound(got, want)
            lost = np.isneginf(got[:, wide])
            shallowest = np.min(neg_bits[lost], initial=np.inf)
            print(f"wide class, {name}: {int((~lost).sum())} pairs of wide reads kept / {int(lost.sum())} -inf (read {r}: "
                  f"{int(np.isneginf(got[:, r]).sum())} of {len(cuts)} -inf); shallowest -inf pair {shallowest:.0f} bits, "
                  f"deepest kept {np.max(neg_bits[~lost], initial=0.0):.0f} bits; kept pairs max |GPU - oracle| {dev:.3e}")
            assert ok, (name, dev)
            assert (~lost).sum() >= 10 and lost.sum() >= 10, name
        forms = _full_forms(gm, rc, mp, cands, models)
        assert _wide_stats()[1] > 0
        for name, got in forms:
            print(f"wide class, {name}, fallback on: max |GPU - oracle| {_maxdiff(got, want):.3e}")
            assert np.array_equal(np.isneginf(got), np.isneginf(want)) and _maxdiff(got, want) <= TOL, name
