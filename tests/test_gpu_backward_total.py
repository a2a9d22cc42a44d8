"""Per-read backward totals of generate_mappings (Mappings.read_logp_backward): B.tables[0].mb of the pass behind the
lists, PHMMOutput::to_full_prob_backward (table.rs:492-494) -- backward_by_forward without input mappings
(backward.rs:101-142), backward_with_mapping with them (backward.rs:59-90), begin states as in backward.rs:499-555.

Against the oracle's run_sparse_adaptive / run_with_mapping, between the kernel classes, across the hand-offs of long
reads, and the reference's own check 2 (hmmv2/tests/dbg.rs:170-172, 229-233): |ln P_fwd - ln P_bwd| < 0.01 per read.
Small read sets only: the whole file is meant to take well under a minute on the GPU."""
import os

import numpy as np
import pytest

import dbgphmm_amd as D
from dbgphmm_amd import _ffi
from fuzz_cases import make_case, make_case_medium
from helpers import scores_tie_aware, subset_csr
from repeat_cases import dataset

pytestmark = pytest.mark.gpu

ACCEPTABLE_ERROR_FORWARD_AND_BACKWARD = 0.01  # dbg.rs:44


def _adaptive(oracle, arrays, reads, use_max_ratio, idx=None, env=None):
    """generate_mappings without input mappings (under the environment `env`); the backward total of every read in `idx`
    that is not a forced switch against the oracle's run_sparse_adaptive (tie-aware, 1e-6).
    -> (model, oracle model, reads, mappings, flags)"""
    gm, om = D.PHMMModel(arrays), oracle.Model(arrays)
    rc = D.ReadCollection(reads)
    os.environ.update(env or {})
    try:
        mp, _ = gm.generate_mappings(rc, None, use_max_ratio)
    finally:
        for v in env or {}:
            os.environ.pop(v, None)
    # (the flags are kept by the score-ratio mode only)
    flags = rc.last_call_info()[1] if use_max_ratio else np.zeros(len(reads), dtype=np.uint32)
    tot, lb = mp.read_logp_backward()
    assert np.all(np.isfinite(lb)) and abs(tot - lb.sum()) <= 1e-9 * max(1.0, abs(tot))
    idx = np.arange(len(reads)) if idx is None else np.asarray(idx)
    # a forced switch continues from the best 400 nodes of a nearly flat column: not a parity target
    keep = [int(i) for i in idx if not flags[i] & _ffi.PHMM_READ_FORCED_SWITCH]

    def want(i):
        return om.run_sparse_adaptive(reads[i], use_max_ratio).to_full_prob_backward()
    if keep:
        scores_tie_aware(oracle, lb[keep], np.array([want(i) for i in keep]), lambda b: want(keep[b]))
    return gm, om, rc, mp, flags


def _hinted(oracle, gm, om, rc, reads, mp, idx):
    """generate_mappings on the GPU's own lists against the oracle's run_with_mapping on the same lists (1e-9)"""
    mh, _ = gm.generate_mappings(rc, mp, True)
    lbh = mh.read_logp_backward()[1]
    off = rc.offsets.astype(np.int64)
    arr = mp.arrays()
    for i in idx:
        m1 = oracle.Mapping(*subset_csr(off, arr, [int(i)]))
        o = om.run_with_mapping(reads[int(i)], m1).to_full_prob_backward()
        assert abs(lbh[i] - o) < 1e-9, (int(i), float(lbh[i]), o)
    return mh


def _check2(oracle, om, reads, mp, use_max_ratio=True):
    """dbg.rs:170-172, 229-233 as written.  A read over the bar must be one the oracle puts over it too; it is then held
    to the oracle's backward total instead.  -> indices of such reads"""
    lf, lb = mp.read_logp()[1], mp.read_logp_backward()[1]
    gap = np.abs(lf - lb)
    over = np.flatnonzero(~(gap < ACCEPTABLE_ERROR_FORWARD_AND_BACKWARD))
    for i in over:
        o = om.run_sparse_adaptive(reads[i], use_max_ratio)
        of, ob = o.to_full_prob_forward(), o.to_full_prob_backward()
        assert abs(of - ob) >= ACCEPTABLE_ERROR_FORWARD_AND_BACKWARD, (int(i), float(lf[i]), float(lb[i]), of, ob)
        scores_tie_aware(oracle, lb[i:i + 1], np.array([ob]),
                         lambda b: om.run_sparse_adaptive(reads[i], use_max_ratio).to_full_prob_backward())
    return over


def test_adaptive_fuzz_cases_match_oracle(gpu_lib, oracle):
    """Both use_max_ratio modes on small random graphs; reads cut short (ends inside the warm-up: column 0 of the dense
    head only, no sparse tail) are part of the cases."""
    rng = np.random.default_rng(20261016)
    short = 0
    for case in range(6):
        c = make_case(rng, case)
        arrays, reads = c["arrays"], list(c["reads"])
        reads.append(reads[0][: max(1, arrays.param.n_warmup // 2)])  # shorter than n_warmup: never switches
        for umr in (True, False):
            gm, om, rc, mp, flags = _adaptive(oracle, arrays, reads, umr)
        short += sum(len(r) < arrays.param.n_warmup for r in reads)
        _hinted(oracle, gm, om, rc, reads, mp, range(len(reads)))
    assert short >= 6


def test_adaptive_medium_cases_and_deferred_reads(gpu_lib, oracle):
    """Several read groups.  The main plan keeps 6 dense columns here (PHMM_WARM_COLS=6, PHMM_NO_KEEP_ALL=1; a read set
    this small otherwise keeps them all), so every read still dense at column 6 is deferred (PHMM_READ_DEFERRED) to
    the all-columns plan on the side worker; reads with a random 22-base prefix are among them."""
    rng = np.random.default_rng(20261017)
    deferred = 0
    for case in range(2):
        c = make_case_medium(rng, case)
        arrays, reads, pick = c["arrays"], list(c["reads"]), [int(p) for p in c["pick"]]
        junk = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(case).integers(0, 4, size=(3, 22))]
        for j in range(3):
            reads.append(junk[j].tobytes() + reads[j])
        gm, om, rc, mp, flags = _adaptive(oracle, arrays, reads, True, idx=pick,
                                          env={"PHMM_WARM_COLS": "6", "PHMM_NO_KEEP_ALL": "1"})
        dfx = [i for i in range(len(reads)) if flags[i] & _ffi.PHMM_READ_DEFERRED and not flags[i] & _ffi.PHMM_READ_FORCED_SWITCH]
        dfx = dfx[:4] + [i for i in dfx if i >= len(reads) - 3]
        lb = mp.read_logp_backward()[1]

        def want(i):
            return om.run_sparse_adaptive(reads[i], True).to_full_prob_backward()
        scores_tie_aware(oracle, lb[dfx], np.array([want(i) for i in dfx]), lambda b: want(dfx[b]))
        deferred += len(dfx)
        _hinted(oracle, gm, om, rc, reads, mp, pick[:6] + dfx)
        _check2(oracle, om, reads, mp)
    assert deferred >= 1


@pytest.mark.parametrize("name,k", [("u1k", 40), ("u100", 40), ("u20", 40), ("u20", 100)])
def test_forward_backward_check2_repeats(gpu_lib, oracle, name, k):
    arrays, reads, sg, haps = dataset(name, k)
    gm, om = D.PHMMModel(arrays), oracle.Model(arrays)
    rc = D.ReadCollection(reads)
    mp, _ = gm.generate_mappings(rc, None, True)
    over = _check2(oracle, om, reads, mp)
    print(f"\n{name} k={k}: reads {len(reads)}, over the 0.01 bar {len(over)}, "
          f"max |fwd-bwd| {np.abs(mp.read_logp()[1] - mp.read_logp_backward()[1]).max():.3g}")


def _u20n200_sample():
    arrays, reads, sg, haps = dataset("u20n200", 40)
    rng = np.random.default_rng(5)
    pick = rng.choice(len(reads), 40, replace=False)
    return arrays, [reads[int(i)] for i in pick]


def test_u20n200_check2_and_kernel_classes(gpu_lib, oracle):
    """40 reads of u20n200 (forced switches and 400-slot positions: the wide kernel runs).  Check 2; the oracle on the
    reads that are not forced switches; default kernels, PHMM_NO_LEAN=1 and PHMM_NO_WIDE_CLASS=1 agree to 1e-9."""
    arrays, reads = _u20n200_sample()
    gm, om, rc, mp, flags = _adaptive(oracle, arrays, reads, True)
    over = _check2(oracle, om, reads, mp)
    print(f"\nu20n200 sample: forced {int(((flags & _ffi.PHMM_READ_FORCED_SWITCH) != 0).sum())}, "
          f"wide {int(((flags & _ffi.PHMM_READ_WIDE_FRONTIER) != 0).sum())}, over the 0.01 bar {len(over)}")
    base = mp.read_logp_backward()[1].copy()
    for var in ("PHMM_NO_LEAN", "PHMM_NO_WIDE_CLASS"):
        os.environ[var] = "1"
        try:
            mv, _ = D.PHMMModel(arrays).generate_mappings(D.ReadCollection(reads), None, True)
            lbv = mv.read_logp_backward()[1]
        finally:
            os.environ.pop(var, None)
        assert np.max(np.abs(lbv - base)) < 1e-9, (var, float(np.max(np.abs(lbv - base))))


def test_long_reads_handoffs(gpu_lib, oracle):
    """10 kb reads: longer than the 6 144-base slice, so the sparse backward walks in slices and bursts and the column
    (with its InsBegin) travels through the hand-off slot."""
    arrays, reads, sg, haps = dataset("sim_n4", 40, coverage=10, read_len=10000, p=0.0003, max_reads=6)
    assert len(reads) >= 4 and max(len(r) for r in reads) > 6144
    gm, om, rc, mp, flags = _adaptive(oracle, arrays, reads, True)
    _check2(oracle, om, reads, mp)
    _hinted(oracle, gm, om, rc, reads, mp, range(2))


def test_plumbing(gpu_lib, oracle):
    c = make_case(np.random.default_rng(20261018), 0)
    arrays, reads = c["arrays"], c["reads"]
    gm = D.PHMMModel(arrays)
    rc = D.ReadCollection(reads)
    mp, _ = gm.generate_mappings(rc, None, True)
    tot, lb = mp.read_logp_backward()
    # twice on the same handle: the same bits; into a caller's buffer
    out = np.empty(len(reads))
    tot2, lb2 = mp.read_logp_backward(out)
    assert lb2 is out and np.array_equal(lb, lb2) and tot == tot2
    # map_nodes carries the values over unchanged (identity node map)
    n = arrays.n_nodes
    mm = mp.map_nodes(gm, np.arange(n + 1, dtype=np.uint32), np.arange(n, dtype=np.uint32))
    assert np.array_equal(mm.read_logp_backward()[1], lb)
    # host-built mappings have no backward pass behind them
    po, nd, lp = mp.arrays()
    host = D.Mappings.from_arrays(rc, po, nd, lp)
    with pytest.raises(Exception):
        host.read_logp_backward()
    # a read scored alone and inside the full set
    for i in (0, len(reads) - 1):
        m1, _ = gm.generate_mappings(D.ReadCollection([reads[i]]), None, True)
        v = m1.read_logp_backward()[1][0]
        assert abs(v - lb[i]) <= 1e-10 * abs(lb[i]), (i, float(v), float(lb[i]))
