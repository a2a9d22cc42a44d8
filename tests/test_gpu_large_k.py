"""Parity in the regime n_warmup = k >= 250 (the reference runs generate_mappings with n_warmup = k while k grows from
40 to thousands: multi_dbg.rs:1394-1409, posterior.rs:735-810): dense heads of hundreds of kept columns, switch columns
past 255 in the uint16 that carries them, natural late switches with 200-400 nodes, read ends at the seam
n_warmup - 1 ... n_warmup + 3, k longer than the reads, and the fixed mode with head and tail of 300 columns.

The read sets and their classes come from large_k_cases (picked by property through the oracle; what they hold is
asserted without a GPU in test_large_k_cases_cpu.py).  Every test prints the switch columns of its reads, the worst
|d ln P| forward and backward, the tie retries and the deferred reads of every plan variant.

Wall time of the file on an MI355X, oracle included (16 threads): 30 s, 2 to 9 s per test; the whole -m gpu suite
takes 12 minutes.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import dbgphmm_amd as D
import large_k_cases as LK
from dbgphmm_amd import _ffi
from helpers import TIE_RULES, compare_mappings_tie_aware, finite_close, same_mappings, scores_tie_aware, subset_csr
from test_gpu_backward_total import _check2, _hinted

pytestmark = pytest.mark.gpu

FORCED, DEFERRED = _ffi.PHMM_READ_FORCED_SWITCH, _ffi.PHMM_READ_DEFERRED
STATS_DENSE_BWD = 1
TOL_USAGE = 1e-7  # node usage of one read, summed over the nodes


def _call(arrays, reads, env=None, gm=None, rc=None):
    """generate_mappings(rc, None, True) under the environment `env` -> what the call returned, copied"""
    gm, rc = gm or D.PHMMModel(arrays), rc or D.ReadCollection(reads)
    os.environ.update(env or {})
    try:
        mp, nf = gm.generate_mappings(rc, None, True)
        cells = _ffi.last_call_stats(STATS_DENSE_BWD)[2]
    finally:
        for v in env or {}:
            os.environ.pop(v, None)
    cols, flags = rc.last_call_info()
    return dict(gm=gm, rc=rc, mp=mp, nf=nf.copy(), arrays=tuple(x.copy() for x in mp.arrays()),
                lf=mp.read_logp()[1].copy(), lb=mp.read_logp_backward()[1].copy(), cols=cols.astype(np.int64),
                flags=flags.copy(), cells=cells)


def _same_bits(a, b):
    """two calls on the same reads: ln P forward and backward and node usage bit-equal, lists by same_mappings"""
    assert np.array_equal(a["lf"], b["lf"]) and np.array_equal(a["lb"], b["lb"])
    assert same_mappings(a["arrays"], b["arrays"])
    assert np.array_equal(a["nf"], b["nf"])


def _usage(csr, n_nodes):
    """Mappings::to_node_freqs (hint.rs:161-171) of one CSR triple"""
    return np.bincount(csr[1], weights=np.exp(csr[2]), minlength=n_nodes)


def _usage_tie_aware(oracle, om, sub, gsub, omp):
    """Node usage of every read from the GPU's lists against the same from the oracle's, sum over the nodes of |d| below
    TOL_USAGE; a read over it is run again through the oracle under the other tie orders (helpers.TIE_RULES) and must
    meet one of them -> (worst sum |d| of a read, reads that needed another tie order)"""
    import ctypes as C
    L = oracle.lib()
    L.orc_set_tie_rule.argtypes = [C.c_double, C.c_int]
    off = np.concatenate([[0], np.cumsum([len(r) for r in sub])])
    n, worst, retried = om.n_nodes, 0.0, 0
    for j, r in enumerate(sub):
        g = _usage(subset_csr(off, gsub, [j]), n)
        d = float(np.abs(g - _usage(subset_csr(off, omp, [j]), n)).sum())
        if not d < TOL_USAGE:
            retried += 1
            seen = [d]
            for eps, rev in TIE_RULES:
                L.orc_set_tie_rule(eps, rev)
                try:
                    o1, _ = om.generate_mappings([r], None, True, n_threads=1)
                finally:
                    L.orc_set_tie_rule(0.0, 0)
                d = float(np.abs(g - _usage(o1, n)).sum())
                seen.append(d)
                if d < TOL_USAGE:
                    break
            else:
                raise AssertionError((j, seen))
        worst = max(worst, d)
    return worst, retried


def _hold_to_oracle(oracle, tag, arrays, reads, ocols, sample, run=None):
    """One generate_mappings(rc, None, True) call on `reads` against the oracle:
    - the switch column of EVERY read (last_call_info) equals the oracle's number of dense forward tables `ocols`
      (len(read) for a read that never switches); at most one read may differ, and only where large_k_cases.dispute
      allows it (the node count crosses warmup_threshold with nodes within 1e-6 nats of the ratio cut)
    - no read is a forced switch: all are parity targets
    and on the reads `sample`:
    - forward and backward total against run_sparse_adaptive, tie-aware at 1e-6; the reference's check 2
    - the mapping lists with compare_mappings_tie_aware, retried share bounded by max(2, 0.1 n)
    - node usage per read from the lists against Mappings::to_node_freqs of the oracle's lists: sum over the nodes of
      |d| < 1e-7 (the bar transfers: measured on an MI355X on these sets 0.9e-9 to 1.9e-9, no read retried)
    - the hinted pass and the list pass on the GPU's own lists against full_prob_reads / run_with_mapping on the same
      lists at 1e-9; the score-only call returns the bits of read_logp
    -> the call"""
    run = run or _call(arrays, reads)
    gm, rc, mp = run["gm"], run["rc"], run["mp"]
    om = oracle.Model(arrays)
    sample = np.asarray(sample, dtype=np.int64)
    print(f"\n{tag}: N={arrays.n_nodes} n_warmup={arrays.param.n_warmup} reads={len(reads)} sample={sample.tolist()}")
    print(f"  switch columns (GPU)    {run['cols'].tolist()}\n  switch columns (oracle) {np.asarray(ocols).tolist()}")
    print(f"  deferred {int(((run['flags'] & DEFERRED) != 0).sum())}, workspace {_ffi.lib().phmm_workspace_bytes() / 2 ** 30:.2f} GiB")
    assert not np.any(run["flags"] & FORCED)
    assert np.all(np.isfinite(run["lf"])) and np.all(np.isfinite(run["lb"]))
    differ = np.flatnonzero(run["cols"] != np.asarray(ocols))
    for i in differ:
        d = LK.dispute(oracle, om, reads[i], run["cols"][i], ocols[i])
        print(f"  read {i}: GPU switches at {run['cols'][i]}, the oracle at {ocols[i]}: {d}")
        assert d["allowed"], (int(i), d)
    assert differ.size <= 1
    # totals
    sub = [reads[i] for i in sample]
    with ThreadPoolExecutor(16) as ex:
        tot = list(ex.map(lambda r: (lambda o: (o.to_full_prob_forward(), o.to_full_prob_backward()))(om.run_sparse_adaptive(r, True)), sub))
    of, ob = np.array([t[0] for t in tot]), np.array([t[1] for t in tot])
    glf, glb = run["lf"][sample], run["lb"][sample]
    print(f"  worst |d ln P| forward {np.abs(glf - of).max():.3e} backward {np.abs(glb - ob).max():.3e}, "
          f"|fwd - bwd| of the sample GPU {np.abs(glf - glb).max():.3e} oracle {np.abs(of - ob).max():.3e}")
    t_f = scores_tie_aware(oracle, glf, of, lambda b: om.run_sparse_adaptive(sub[b], True).to_full_prob_forward())
    t_b = scores_tie_aware(oracle, glb, ob, lambda b: om.run_sparse_adaptive(sub[b], True).to_full_prob_backward())
    over = _check2(oracle, om, reads, mp)
    # lists and node usage
    omp, _ = om.generate_mappings(sub, None, True, n_threads=16)
    gsub = subset_csr(rc.offsets.astype(np.int64), run["arrays"], sample)
    t_l, overflow = compare_mappings_tie_aware(oracle, om, sub, gsub, omp, ratio=arrays.param.active_node_max_ratio)
    worst_u, t_u = _usage_tie_aware(oracle, om, sub, gsub, omp)
    print(f"  tie retries: forward {t_f} backward {t_b} lists {t_l} usage {t_u}; overflow reads {overflow}; over the 0.01 bar "
          f"{len(over)}; worst node usage sum |d| of a read {worst_u:.3e}")
    bound = max(2, 0.1 * len(sub))
    assert overflow == 0 and t_f + t_l <= bound and t_b <= bound and t_u <= bound, (t_f, t_b, t_l, t_u, overflow)
    # (the call's node usage is that of its lists)
    assert np.max(np.abs(mp.to_node_freqs(arrays.n_nodes) - run["nf"])) < 1e-9
    assert abs(run["nf"].sum() - rc.total_bases()) < 0.02 * rc.total_bases()
    # the passes on the GPU's own lists
    mh = _hinted(oracle, gm, om, rc, reads, mp, sample)
    olp_h = om.full_prob_reads(sub, gsub, True, n_threads=16)
    _, lp_h = gm.to_full_prob_reads(rc, mp)
    d_h, d_l = np.abs(lp_h[sample] - olp_h).max(), np.abs(mh.read_logp()[1][sample] - olp_h).max()
    print(f"  on its own lists: hinted pass |d ln P| {d_h:.3e}, list pass {d_l:.3e}")
    assert d_h < 1e-9 and d_l < 1e-9
    _, lp_s = gm.to_full_prob_reads(rc, None, True)
    assert np.array_equal(lp_s, run["lf"])
    return run


@pytest.mark.parametrize("name,k", [("u100n100", 270), ("u100n100", 300), ("u20n200", 300)])
def test_late_natural_switches_match_oracle(gpu_lib, oracle, name, k):
    """Items 1 and 2 on the first 12 / 24 / 24 reads: natural switches at columns 78 ... 292 with 200-400 nodes, at
    k = 270 two reads that switch exactly at n_warmup."""
    c = LK.classes(oracle, name, k)
    run = _hold_to_oracle(oracle, f"{name} k={k}", c["arrays"], c["reads"], c["cols"], LK.oracle_sample(c))
    if name == "u100n100":
        assert run["cols"].max() > 255
    if k == 270:
        assert (run["cols"] == k).sum() >= 2


def _deferred(run):
    return (run["flags"] & DEFERRED) != 0


def test_plans_agree(gpu_lib, oracle):
    """The k = 270 set under every plan: all 272 columns kept by the main plan (default), by the side plan beside it
    or queued behind it, a main plan of 200 columns, several chunks and workers, a second call sorted by hints above
    255, a workspace limit, the dense backward with and without its skip -- same bits; the kernel classes to 1e-9."""
    c = LK.classes(oracle, "u100n100", 270)
    arrays, reads, k = c["arrays"], c["reads"], 270
    base = _call(arrays, reads)
    ws = int(_ffi.lib().phmm_workspace_bytes())
    lens = np.array([len(r) for r in reads], dtype=np.int64)
    cols = base["cols"]
    print(f"\nswitch columns {cols.tolist()}, workspace after the default call {ws / 2 ** 30:.2f} GiB")
    assert cols.max() > 255 and (cols == k).sum() >= 2
    assert not np.any(_deferred(base))  # the lc_full branch: nothing deferred with all n_warmup + 2 columns kept

    def variant(tag, env, ref=base, **kw):
        r = _call(arrays, reads, env, **kw)
        print(f"{tag}: deferred {int(_deferred(r).sum())} of {len(reads)}")
        assert np.array_equal(r["cols"], cols)
        if ref is not None:
            _same_bits(ref, r)
        return r

    # the main plan keeps its ~16 columns: every read here is still dense there and goes to the 272-column side plan
    assert cols.min() > 40
    assert np.all(_deferred(variant("PHMM_NO_KEEP_ALL", {"PHMM_NO_KEEP_ALL": "1"})))
    assert np.all(_deferred(variant("PHMM_NO_KEEP_ALL, no side worker", {"PHMM_NO_KEEP_ALL": "1", "PHMM_NO_SIDE_WORKER": "1"})))
    r = variant("PHMM_NO_KEEP_ALL, PHMM_WARM_COLS=200", {"PHMM_NO_KEEP_ALL": "1", "PHMM_WARM_COLS": "200"})
    assert np.array_equal(_deferred(r), cols >= 200) and 0 < _deferred(r).sum() < len(reads)
    # (twelve reads are one group of 16 lanes: groups of four make three of them for the chunks and the workers)
    variant("three chunks", {"PHMM_DENSE_W": "4", "PHMM_CHUNK_GROUPS": "1"})
    variant("three workers", {"PHMM_DENSE_W": "4", "PHMM_WORKERS": "3", "PHMM_CHUNK_GROUPS": "1", "PHMM_PIPELINE_MIN_GROUPS": "2"})
    # a second call on the same ReadCollection: the plan is sorted by hints above 255
    variant("second call on the same reads", None, gm=base["gm"], rc=base["rc"])
    # a workspace limit under which the tables of the three groups of four reads no longer fit one chunk
    per_group = (k + 2) * arrays.n_nodes * 4 * 24
    limit = min(ws // 2, per_group * 3 // 2)
    _ffi.check(_ffi.lib().phmm_set_workspace_limit(limit))
    try:
        variant(f"workspace limit {limit / 2 ** 30:.2f} GiB", {"PHMM_DENSE_W": "4"})
    finally:
        _ffi.check(_ffi.lib().phmm_set_workspace_limit(0))
    print(f"workspace after the limited call {_ffi.lib().phmm_workspace_bytes() / 2 ** 30:.2f} GiB")
    # The dense-head backward with its run / segment masks and without, W = 64.  Reads whose frontier outgrows the
    # one-lane-per-node class (7 of these 12) leave the main plan for a plan of their own, whose launches the statistics
    # leave out as they do the deferred plan's: the pair is run with that hand-over (bits) and without it
    # (PHMM_NO_WIDE_HANDOVER=1: bits, and the count of every dense backward cell of every read).
    dense = int(np.where(cols < lens, cols + 1, lens).sum()) * arrays.n_nodes
    for npt, extra in ((2, {"PHMM_NO_WIDE_HANDOVER": "1"}), (8, {"PHMM_NO_WIDE_HANDOVER": "1"}), (8, {})):
        env = dict({"PHMM_DENSE_W": "64", "PHMM_DENSE_NPT": str(npt)}, **extra)
        # (another run length sums the dense columns in another order: list values move in the last bits against the
        # default call, so this pair is held to each other, and its totals to the default call's at 1e-9)
        on = variant(f"W=64 npt={npt} {'no hand-over ' if extra else ''}skip", env, ref=None)
        assert np.abs(on["lf"] - base["lf"]).max() < 1e-9 and np.abs(on["lb"] - base["lb"]).max() < 1e-9
        off = variant(f"W=64 npt={npt} {'no hand-over ' if extra else ''}no skip", dict(env, PHMM_NO_BWD_SKIP="1"), ref=on)
        assert not np.any(_deferred(on)) and not np.any(_deferred(off))
        print(f"dense backward cells: skip {on['cells']}, no skip {off['cells']}, dense count {dense}")
        assert 0 < on["cells"] < off["cells"]
        if extra:
            assert off["cells"] == dense
    # the kernel classes of the sparse tail
    for var in ("PHMM_NO_LEAN", "PHMM_NO_WIDE_CLASS"):
        r = _call(arrays, reads, {var: "1"})
        d_f, d_b = np.abs(r["lf"] - base["lf"]).max(), np.abs(r["lb"] - base["lb"]).max()
        print(f"{var}: |d ln P| forward {d_f:.3e} backward {d_b:.3e}")
        assert d_f < 1e-9 and d_b < 1e-9 and np.array_equal(r["cols"], cols)


def test_seam_lengths(gpu_lib, oracle):
    """A read that switches at n_warmup cut to n_warmup - 1 ... n_warmup + 3 bases, two cuts that never switch and the
    two uncut reads in one call (min_len <= n_warmup + 2: three emit-prob planes, the plane of merged index len is
    written), every read against the oracle; then the uncut reads alone (two planes): the same bits."""
    c = LK.classes(oracle, "u100n100", 270)
    arrays, k = c["arrays"], 270
    cuts, names = LK.seam_reads(c)
    uncut = [c["reads"][int(c["at_warmup"][0])], c["reads"][int(max(c["above_255"], key=lambda i: c["cols"][i]))]]
    reads = cuts + uncut
    ocols = LK.switches(oracle, oracle.Model(arrays), reads)[0]
    print("\n" + "; ".join(names))
    a = _hold_to_oracle(oracle, "seam lengths k=270", arrays, reads, ocols, np.arange(len(reads)))
    lens = np.array([len(r) for r in reads])
    assert a["cols"][:7].tolist() == [k - 1, k, k, k, k, 150, lens[6]] and np.all(a["cols"][[0, 1, 5, 6]] == lens[[0, 1, 5, 6]])
    b = _call(arrays, uncut)
    at = np.array([len(cuts), len(cuts) + 1])
    assert np.array_equal(b["lf"], a["lf"][at]) and np.array_equal(b["lb"], a["lb"][at]) and np.array_equal(b["cols"], a["cols"][at])
    assert same_mappings(b["arrays"], subset_csr(a["rc"].offsets.astype(np.int64), a["arrays"], at))


def test_k_longer_than_the_reads(gpu_lib, oracle):
    """n_warmup = k = 1100 on reads of 1000 bases: the kept columns and the ln(ib) tables are bounded by the read
    length; the reads still switch, near columns 305-350; one read cut to 280 bases never does."""
    c = LK.classes(oracle, "u100n100", 1100)
    reads = list(c["reads"]) + [c["reads"][0][:280]]
    ocols = np.concatenate([c["cols"], [280]])
    run = _hold_to_oracle(oracle, "u100n100 k=1100", c["arrays"], reads, ocols, np.arange(len(reads)))
    assert np.all((run["cols"][:4] >= 290) & (run["cols"][:4] <= 360)) and run["cols"][4] == 280


def test_fixed_mode_n_warmup_300(gpu_lib, oracle):
    """use_max_ratio = 0 with n_active_nodes = 200 at n_warmup = 300: dense head (forward) and dense tail (backward) of
    300 columns each on reads of 1000, 600 (head and tail overlap), 300, 299 and 150 bases -- to_full_prob_reads,
    to_full_prob_sparse_backward and run_sparse against the oracle (tie-aware, 1e-6; node usage as
    test_gpu_sparse.py holds run_sparse: 1e-9 per read), and every column of backward_sparse of the 600-base read at
    the bar of test_backward_sparse_tables_match_oracle (finite_close, 1e-8).

    The 600-base read is picked by property (large_k_cases.tie_stable_cut): the first read of the set whose tables the
    reference pins.  On this repeat the top-200 cut of backward_sparse meets equal values at 28 to 115 of the
    300 sparse columns of such a read.  Values equal to the last bit stay in storage order in the oracle and in the kernels alike; values
    that differ by rounding noise only make the oracle's OWN tables depend on its tie rule -- on read 1 cut to 600 the
    oracle against itself differs in 412 to 698 of the 1 800 (column, table) pairs at 1e-8, and the GPU misses the
    default order in 412 and the nearest rule in 9 (worst entry 5.0e-7, 27 nats under the best of its column; flags,
    Begin states and totals agree).  One read of the first eight has no such decision; its tables are held in full."""
    c = LK.classes(oracle, "u100n100", 300)
    arrays = D.vectorised_to_phmm(c["sg"], c["arrays"].param.with_(n_active_nodes=200), 1)
    src = c["reads"]
    gm, om = D.PHMMModel(arrays), oracle.Model(arrays)
    pinned, stable = LK.tie_stable_cut(oracle, om, src[:8], 600)
    print(f"\n600-base cuts whose backward_sparse tables the reference pins: {stable}")
    assert pinned is not None
    reads = [src[0], src[pinned][:600], src[2][:300], src[3][:299], src[4][:150]]
    assert len(reads[0]) >= 997 and len(reads[1]) == 600 and arrays.param.n_warmup == 300
    rc = D.ReadCollection(reads)
    _, lp = gm.to_full_prob_reads(rc, None, False)
    olp = om.full_prob_reads(reads, None, False, n_threads=16)
    t0 = scores_tie_aware(oracle, lp, olp, lambda b: om.full_prob_reads([reads[b]], None, False, n_threads=1)[0])
    _, lpb = gm.to_full_prob_sparse_backward(rc)
    with ThreadPoolExecutor(16) as ex:
        outs = list(ex.map(om.run_sparse, reads))
    olf, olb = np.array([o.to_full_prob_forward() for o in outs]), np.array([o.to_full_prob_backward() for o in outs])
    t1 = scores_tie_aware(oracle, lpb, olb, lambda b: om.backward(reads[b], oracle.BWD_SPARSE).full_prob())
    lf, lb, nf = gm.run_sparse(rc)
    t2 = scores_tie_aware(oracle, lf, olf, lambda b: om.run_sparse(reads[b]).to_full_prob_forward())
    t3 = scores_tie_aware(oracle, lb, olb, lambda b: om.run_sparse(reads[b]).to_full_prob_backward())
    print(f"\nfixed mode: worst |d ln P| to_full_prob_reads {np.abs(lp - olp).max():.3e}, sparse backward {np.abs(lpb - olb).max():.3e}, "
          f"run_sparse forward {np.abs(lf - olf).max():.3e} backward {np.abs(lb - olb).max():.3e}; tie retries {t0} {t1} {t2} {t3}")
    # state_probs = sum over the merged indices of the emit probs (freq.rs:236-243), without the 400-element capacity
    # of a sparse accumulator (see test_run_sparse_node_freqs_match_oracle)
    onf = np.zeros(arrays.n_nodes)
    for o, r in zip(outs, reads):
        for jj in range(len(r) + 1):
            m, i, d, _ = o.to_emit_probs(jj)
            onf += np.exp(m) + np.exp(i) + np.exp(d)
    print(f"run_sparse node usage: max |d| {np.abs(nf - onf).max():.3e}")
    assert np.max(np.abs(nf - onf)) < 1e-9 * len(reads)
    assert abs(nf.sum() - rc.total_bases()) < 0.02 * rc.total_bases()
    # backward_sparse of the 600-base read (shorter than 2 n_warmup): every column
    read = reads[1]
    gt, dense = gm.backward_sparse(read)
    ot = outs[1].backward
    L = len(read)
    assert dense.tolist() == [ot.is_dense(i) for i in range(L)] and dense.sum() == 300
    for i in range(L):
        m, ins, d, s = ot.table(i)
        for name, g, o in (("m", gt.m[i], m), ("i", gt.i[i], ins), ("d", gt.d[i], d)):
            floor = np.max(o) - 600.0 if dense[i] else None  # the dense kernel's scaled linear range
            assert np.all(finite_close(g, o, 1e-8, floor)), (i, name, dense[i])
        assert abs(gt.scal[i, 0] - s[0]) < 1e-8 and abs(gt.scal[i, 1] - s[1]) < 1e-8, (i, gt.scal[i], s)
    assert abs(gt.scal[0, 0] - ot.full_prob()) < 1e-8
