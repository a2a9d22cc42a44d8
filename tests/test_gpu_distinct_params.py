"""GPU: every kernel family against the oracle under parameters whose fifteen probabilities all differ.

Every other parameter set of the suite has p_MI = p_MD = p_ID = p_DI, p_II = p_DD, p_IM = p_DM, p_random = ln 1/4 and
p_match = ln(1 - p_mismatch), and each kernel family copies the fifteen fields by hand into a struct of its own: two
tied fields exchanged in one of these copies, a hard-coded 0.25 or a 1 - mismatch computed on the device pass everything
else.  Here each family runs once on tests/distinct_params.py's set and fixtures and is held to the oracle (or, for the
walks, to the Python restatements, which index the nine transitions separately and are pinned by enumeration over random
parameters on the CPU) at the bar its own test file uses:
  ln P 1e-9 for the dense, hinted and list passes and 1e-6 for the adaptive flow; table and posterior entries 1e-8 above
  the ln 1e-12 floor; node usage 1e-7 per read; edge and init frequencies 1e-9 per read; walks, rows and records word for
  word.
tests/test_distinct_params_cpu.py shows that an exchanged pair moves each of these outputs by 100 bars or more, that the
oracle's forward is the sum over all paths under random parameters and its backward the reference's b_step."""
import math

import numpy as np
import pytest

import alignments_ref as A
import best_path_ref as B
import dbgphmm_amd as D
import distinct_params as P
import mea_path_ref as M
import sample_paths_ref as S
import sample_reads_ref as G
from dbgphmm_amd import _ffi
from helpers import compare_mappings, compare_mappings_tie_aware, scores_tie_aware, subset_csr
from test_gpu_edges_wide import _oracle_sums
from test_gpu_list_tables import oracle_tables
from test_gpu_states import oracle_states

pytestmark = pytest.mark.gpu
NINF = -math.inf
LN_FLOOR = math.log(1e-12)
TOL_LOGP = 1e-9    # dense, hinted and list passes, per read
TOL_ADAPT = 1e-6   # the adaptive flow, per read (tie-aware as everywhere)
TOL_EXACT = 1e-6   # the exact dense path (test_gpu_dense.py: test_chimeric_read_takes_the_exact_path)
TOL_ENTRY = 1e-8   # table and posterior entries above the floor
TOL_USAGE = 1e-7   # node usage, per read
TOL_FREQ = 1e-9    # edge and init frequencies, per read (test_gpu_dense.py, test_gpu_hinted_edges.py)
STATS_WIDE = 4     # index of phmm_last_call_stats the block kernels fill
FORCED = _ffi.PHMM_READ_FORCED_SWITCH


def _dev(a, b):
    """largest |a - b|, -inf against -inf counting as equal; NaN if one side is finite where the other is not"""
    a, b = np.asarray(a, float), np.asarray(b, float)
    with np.errstate(invalid="ignore"):
        d = np.where(a == b, 0.0, np.abs(a - b))
    return float(np.max(d, initial=0.0)) if not np.any(np.isnan(d)) else math.nan


def _held(what, d, bar):
    print(f"{what}: worst deviation {d:.3e} (bar {bar:.1e})")
    assert d <= bar, (what, d, bar)  # (NaN fails)


def _fixture(which):
    return P.dbg() if which == "dbg" else P.u20()


def _lists(which, width):
    """(pos_off, nodes) of the oracle's own lists of a fixture, as generated or padded to `width`"""
    return P.lists_of(which)[:2] if width is None else P.padded(which, width)


def _read_lists(po, nd, off, j):
    return B.lists_of(po, nd, off[j], off[j + 1])


def _hold_log_table(what, got, ref):
    """one position's table (entries and scalars together, log space): a value whose oracle value lies within ln 1e-12 of
    the table's largest is held at 1e-8; one below that floor is -inf or below the floor + 1e-8 -> worst deviation"""
    floor = ref.max() + LN_FLOOR
    hi = ref >= floor
    with np.errstate(invalid="ignore"):
        d = np.where(got == ref, 0.0, np.abs(got - ref))
    assert not np.any(np.isnan(got)) and not np.any(np.isnan(d[hi])), what
    assert np.all((got[~hi] == NINF) | (got[~hi] < floor + TOL_ENTRY)), what + ": a value under the floor is too large"
    return float(d[hi].max(initial=0.0))


# ------------------------------------------------------------------ 1. dense
@pytest.mark.parametrize("which", ["dbg", "u20"])
def test_dense_scores_and_node_usage(gpu_lib, oracle, which):
    f = _fixture(which)
    reads = f["reads"]
    lf, lb, nf = D.PHMMModel(f["arrays"]).run_dense(D.ReadCollection(reads))
    olf, olb, onf = oracle.Model(f["arrays"]).run_dense_reads(reads, n_threads=8)
    _held(f"{which}(), dense forward ln P", _dev(lf, olf), TOL_LOGP)
    _held(f"{which}(), dense backward ln P", _dev(lb, olb), TOL_LOGP)
    _held(f"{which}(), dense node usage over {len(reads)} reads", _dev(nf, onf), TOL_USAGE * len(reads))


@pytest.mark.parametrize("gaps", [0, 4, 6])
def test_dense_tables_entry_by_entry(gpu_lib, oracle, gaps):
    """phmm_dense_tables; above n_max_gaps = 4 the merged Del closure folds p_MD, p_ID and p_DD together"""
    f = P.dbg()
    arrays = P.with_param(f["arrays"], P.params(24, gaps))
    gm, om = D.PHMMModel(arrays), oracle.Model(arrays)
    worst = 0.0
    for r in (f["reads"][1][:48], f["reads"][2][:33], P.with_indels(f["reads"][3][:60], 20, 40)):
        out, of, ob = gm.run(r), om.forward(r), om.backward(r)
        for i in range(len(r)):
            for side, T, O in (("forward", out.forward, of), ("backward", out.backward, ob)):
                m, ins, d, s = O.table(i)
                # (the scalars a side does not define are -inf on both: forward mb, backward e)
                got = np.concatenate([T.m[i], T.i[i], T.d[i], T.scal[i]])
                worst = max(worst, _hold_log_table(f"n_max_gaps {gaps}, {side} table {i}", got, np.concatenate([m, ins, d, s])))
    _held(f"dense tables, n_max_gaps {gaps}", worst, TOL_ENTRY)


def _oracle_dense_edges(om, arrays, reads):
    ef, inf = np.zeros(arrays.n_edges), np.zeros(arrays.n_nodes)
    for r in reads:
        e1, n1 = om.run(r).to_edge_and_init_freqs()
        ef += e1
        inf += n1
    return ef, inf


def test_dense_edge_freqs_and_q_score(gpu_lib, oracle):
    f = P.dbg()
    arrays, reads = f["arrays"], f["reads"]
    gm, om = D.PHMMModel(arrays), oracle.Model(arrays)
    lf, ef, inf = gm.run_dense_edge_freqs(D.ReadCollection(reads))
    olf, _, _ = om.run_dense_reads(reads, n_threads=8)
    oef, oinf = _oracle_dense_edges(om, arrays, reads)
    _held("dense edges call, ln P", _dev(lf, olf), TOL_LOGP)
    _held("dense edge frequencies", _dev(ef, oef), TOL_FREQ * len(reads))
    _held("dense init frequencies", _dev(inf, oinf), TOL_FREQ * len(reads))
    # q_score_exact (q.rs:66-96) on the oracle's posteriors, as tests/test_gpu_dense.py evaluates it
    emit = arrays.emission != ord("n")
    ok_e = emit[arrays.edge_src] & emit[arrays.edge_dst]
    assert np.all(np.isfinite(arrays.init_logp[emit])) and np.all(np.isfinite(arrays.trans_logp[ok_e]))
    want_init = float(np.sum(oinf[emit] * arrays.init_logp[emit]))
    want_trans = float(np.sum(oef[ok_e] * arrays.trans_logp[ok_e]))
    qi, qt, qp = gm.q_score_exact(ef, inf)
    print(f"q_score_exact: init {qi:.6f} for {want_init:.6f}, trans {qt:.6f} for {want_trans:.6f}")
    assert qp == 0.0 and abs(qi - want_init) < 1e-6 * max(1.0, abs(want_init))
    assert abs(qt - want_trans) < 1e-6 * max(1.0, abs(want_trans))


def test_the_chimera_stays_on_the_scaled_dense_kernels(gpu_lib, oracle, monkeypatch):
    """reads[0][:60] + reads[1][:100]: 25 nats by the certificate's measure (tests/test_distinct_params_cpu.py), so it is
    certified: with the exact path switched off it is still a number, and it meets the fast path's own bars"""
    f = P.dbg()
    arrays = f["arrays"]
    reads = [f["reads"][2], P.chimera(), f["reads"][3]]
    gm, om, rc = D.PHMMModel(arrays), oracle.Model(arrays), D.ReadCollection(reads)
    monkeypatch.setenv("PHMM_NO_EXACT_DENSE", "1")
    lf, lb, nf = gm.run_dense(rc)
    monkeypatch.delenv("PHMM_NO_EXACT_DENSE")
    assert np.all(np.isfinite(lf))
    olf, olb, onf = om.run_dense_reads(reads, n_threads=4)
    _held("chimera, forward ln P", _dev(lf, olf), TOL_LOGP)
    _held("chimera, backward ln P", _dev(lb, olb), TOL_LOGP)
    _held("chimera, node usage", _dev(nf, onf), TOL_USAGE * len(reads))


def test_exact_dense_path_on_the_deep_chimera(gpu_lib, oracle, monkeypatch):
    """783 nats by the same measure: with PHMM_NO_EXACT_DENSE=1 it comes back NaN, with the fallback it is held to the
    oracle at the bar the exact path is pinned at"""
    arrays, chim = P.deep_chimera()
    f = P.dbg()
    reads = [f["reads"][2], chim, f["reads"][3]]  # (reads of dbg()'s genome: the first 800 bases of this one)
    gm, om, rc = D.PHMMModel(arrays), oracle.Model(arrays), D.ReadCollection(reads)
    monkeypatch.setenv("PHMM_NO_EXACT_DENSE", "1")
    lf0, _, _ = gm.run_dense(rc)
    monkeypatch.delenv("PHMM_NO_EXACT_DENSE")
    print(f"without the exact path: ln P {lf0}")
    assert np.isnan(lf0[1]) and np.all(np.isfinite(lf0[[0, 2]])), "the deep chimera does not take the exact dense path"
    lf, lb, nf = gm.run_dense(rc)
    olf, olb, onf = om.run_dense_reads(reads, n_threads=4)
    _held("exact dense path, forward ln P", _dev(lf, olf), TOL_EXACT)
    _held("exact dense path, backward ln P", _dev(lb, olb), TOL_EXACT)
    _held("exact dense path, node usage", _dev(nf, onf), TOL_EXACT)
    _held("the reads beside it, forward ln P", _dev(lf[[0, 2]], olf[[0, 2]]), TOL_LOGP)
    lf3, ef, inf = gm.run_dense_edge_freqs(rc)
    oef, oinf = _oracle_dense_edges(om, arrays, reads)
    _held("exact dense path, edge and init frequencies", max(_dev(lf3, olf), _dev(ef, oef), _dev(inf, oinf)), TOL_EXACT)


# ------------------------------------------------------------------ 2. hinted forward on the oracle's lists
def _hinted(gm, rc, po, nd):
    return gm.to_full_prob_reads(rc, D.Mappings.from_arrays(rc, po, nd))[1]


def test_hinted_forward_packed_classes(gpu_lib, oracle):
    """lists of at most 8 / 16 / 32 nodes and beyond (the widths of tests/test_gpu_sparse.py), in the full form and as a
    batch of candidates, which is what the packed kernels take"""
    f = P.dbg()
    arrays, reads, sg = f["arrays"], f["reads"], f["sg"]
    om = oracle.Model(arrays)
    per_read = []
    for r, wd in zip(reads, (3, 8, 9, 16, 17, 32, 33, 70)):
        m = om.run(r).to_mapping(wd)
        per_read.append([m.nodes(i) for i in range(len(r))])
    po, nd = B.csr(per_read)
    want = om.full_prob_reads(reads, (po, nd, np.zeros(nd.size)), True, n_threads=8)
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    mp = D.Mappings.from_arrays(rc, po, nd)
    _held("packed widths, full form", _dev(gm.to_full_prob_reads(rc, mp)[1], want), TOL_LOGP)
    cn = sg.copy_num.astype(np.uint32)
    _, lp = gm.to_full_prob_reads_copy_nums(rc, mp, np.stack([cn] * 5), 0)
    _held("packed widths, five candidates", max(_dev(lp[c], want) for c in range(5)), TOL_LOGP)


@pytest.mark.parametrize("width", [None, 64, 65, 400], ids=["as_generated", "pad64", "pad65", "pad400"])
def test_hinted_forward_one_wave_classes(gpu_lib, oracle, width):
    f = P.dbg()
    po, nd = _lists("dbg", width)
    want = oracle.Model(f["arrays"]).full_prob_reads(f["reads"], (po, nd, np.zeros(nd.size)), True, n_threads=8)
    got = _hinted(D.PHMMModel(f["arrays"]), D.ReadCollection(f["reads"]), po, nd)
    _held(f"hinted forward, longest list {int(np.diff(po.astype(np.int64)).max())}", _dev(got, want), TOL_LOGP)


@pytest.mark.parametrize("block", [False, True], ids=["generic", "block"])
def test_hinted_forward_wide_lists(gpu_lib, oracle, monkeypatch, block):
    f = P.u20()
    po, nd, _ = P.lists_of("u20")
    want = oracle.Model(f["arrays"]).full_prob_reads(f["reads"], (po, nd, np.zeros(nd.size)), True, n_threads=8)
    if block:
        monkeypatch.setenv("PHMM_WIDE_HINTED", "1")
    else:
        monkeypatch.setenv("PHMM_NO_WIDE_HINTED", "1")
    got = _hinted(D.PHMMModel(f["arrays"]), D.ReadCollection(f["reads"]), po, nd)
    launches = _ffi.last_call_stats(STATS_WIDE)[1]
    _held(f"hinted forward on u20(), block launches {launches}", _dev(got, want), TOL_LOGP)
    assert (launches > 0) == block


@pytest.mark.parametrize("deep", [False, True], ids=["cut_at_50", "cut_at_170"])
def test_hinted_forward_on_cut_reads(gpu_lib, oracle, monkeypatch, deep):
    """the InsBegin chain (p_random, p_II, p_IM, p_ID) carries the read to the cut.  Cut at base 50 the chain is 223 bits
    under the column before it and the scaled kernels hold it; cut at base 170 of a longer read it is 921 bits under and
    the exact kernel takes the read: with PHMM_NO_EXACT_HINTED=1 it is flagged (-inf), and finite otherwise"""
    c = P.deep_cut_read() if deep else P.cut_read()
    po, nd = c["lists"]
    with np.errstate(divide="ignore"):
        want = oracle.Model(c["arrays"]).full_prob_reads(c["reads"], (po, nd, np.zeros(nd.size)), True, n_threads=1)
    gm, rc = D.PHMMModel(c["arrays"]), D.ReadCollection(c["reads"])
    monkeypatch.setenv("PHMM_NO_EXACT_HINTED", "1")
    scaled = _hinted(gm, rc, po, nd)
    monkeypatch.delenv("PHMM_NO_EXACT_HINTED")
    print(f"cut read without the exact kernel: {scaled}")
    if deep:
        assert np.isneginf(scaled[0]), "the deep cut read does not take the exact hinted kernel"
    else:
        _held("cut read on the scaled kernels", _dev(scaled, want), TOL_LOGP)
    got = _hinted(gm, rc, po, nd)
    assert np.isfinite(got[0])
    _held(f"cut read, ln P {got[0]:.3f}", _dev(got, want), TOL_LOGP)
    # the candidate forms on the uncut model reach the same kernels
    f = P.dbg()
    gm0 = D.PHMMModel(f["arrays"])
    mp = D.Mappings.from_arrays(rc, po, nd)
    base, cut = f["sg"].copy_num.astype(np.uint32), c["sg"].copy_num.astype(np.uint32)
    a = gm0.to_full_prob_reads_copy_nums(rc, mp, cut[None, :], 0)[1][0]
    b = gm0.to_full_prob_reads_copy_num_changes(rc, mp, base, D.copy_num_changes(base, cut[None, :]), 0)[1][0]
    _held("cut read as a candidate, both forms", max(_dev(a, want), _dev(b, want)), TOL_LOGP)


# ------------------------------------------------------------------ 3. candidates
def test_candidate_batch_in_every_form(gpu_lib, oracle):
    f = P.dbg()
    arrays, reads, sg = f["arrays"], f["reads"], f["sg"]
    po, nd, _ = P.lists_of("dbg")
    lists = (po, nd, np.zeros(nd.size))
    rng = np.random.default_rng(20261021)
    base = sg.copy_num.astype(np.uint32)
    listed = np.unique(nd)
    cands = np.repeat(base[None, :], 5, axis=0)
    for c in range(5):
        cands[c, rng.choice(listed, size=6, replace=False)] = rng.integers(0, 4, size=6)
    want = []
    for c in range(5):
        with np.errstate(divide="ignore"):
            a2 = D.vectorised_to_phmm(D.SeqGraph(cands[c].astype(np.int64), sg.base, sg.edge_src, sg.edge_dst, None), arrays.param, 0)
            want.append(oracle.Model(a2).full_prob_reads(reads, lists, True, n_threads=8))
    want = np.stack(want)
    assert np.any(np.abs(want - want[0]) > 1e-3)  # (the candidates differ in what they give the reads)
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    mp = D.Mappings.from_arrays(rc, po, nd)
    changes = D.copy_num_changes(base, cands)
    _held("candidates as copy-number vectors", _dev(gm.to_full_prob_reads_copy_nums(rc, mp, cands, 0)[1], want), TOL_LOGP)
    _held("candidates as changes", _dev(gm.to_full_prob_reads_copy_num_changes(rc, mp, base, changes, 0)[1], want), TOL_LOGP)
    lk = gm.likelihood(rc, mp, base, 0)
    _held("Likelihood.score_changes", _dev(lk.score_changes(changes)[1], want), TOL_LOGP)
    off, node, cn = changes
    lk.move(node[int(off[2]):int(off[3])], cn[int(off[2]):int(off[3])])
    vec, cur, tot = lk.current()
    assert np.array_equal(vec, cands[2])
    _held("Likelihood.move to candidate 2", _dev(cur, want[2]), TOL_LOGP)
    if np.all(np.isfinite(want[2])):
        assert abs(tot - want[2].sum()) <= TOL_LOGP * len(reads)


# ------------------------------------------------------------------ 4. the adaptive flow
@pytest.mark.parametrize("use_max_ratio", [True, False], ids=["ratio", "top_k"])
@pytest.mark.parametrize("knob", [None, "PHMM_NO_LEAN", "PHMM_NO_WIDE_CLASS"])
@pytest.mark.parametrize("which", ["dbg", "u20"])
def test_adaptive_flow(gpu_lib, oracle, monkeypatch, which, knob, use_max_ratio):
    """generate_mappings and to_full_prob_reads without lists; with PHMM_NO_LEAN / PHMM_NO_WIDE_CLASS each restatement
    of the frontier step meets the oracle itself, not only its sibling"""
    f = _fixture(which)
    arrays, reads = f["arrays"], f["reads"]
    if knob:
        monkeypatch.setenv(knob, "1")
    gm, om = D.PHMMModel(arrays), oracle.Model(arrays)
    rc_all = D.ReadCollection(reads)
    gm.to_full_prob_reads(rc_all, None, True)
    forced = (rc_all.last_call_info()[1] & FORCED) != 0
    assert forced.sum() <= (len(reads) // 4 if which == "dbg" else 0), forced
    if not use_max_ratio:
        forced[:] = False  # (the fixed-size mode has no forced switch: it cuts to n_active_nodes everywhere)
    reads = [r for r, x in zip(reads, forced) if not x]
    rc = D.ReadCollection(reads)
    mode = "ratio" if use_max_ratio else "top-k"
    what = f"{which}(), {knob or 'no knob'}, {mode}, {len(reads)} reads"

    def one(b, fn):
        return fn(reads[b])
    olp = om.full_prob_reads(reads, None, use_max_ratio, n_threads=8)
    mp, nf = gm.generate_mappings(rc, None, use_max_ratio)
    lp = mp.read_logp()[1].copy()
    _, lp2 = gm.to_full_prob_reads(rc, None, use_max_ratio)
    assert np.array_equal(lp, lp2)  # the score-only flow walks the same plans
    t0 = scores_tie_aware(oracle, lp, olp, lambda b: om.full_prob_reads([reads[b]], None, use_max_ratio, n_threads=1)[0], tol=TOL_ADAPT)
    omp, onf = om.generate_mappings(reads, None, use_max_ratio, n_threads=8)
    kw = dict(ratio=arrays.param.active_node_max_ratio) if use_max_ratio else dict(top_k=arrays.param.n_active_nodes)
    t1, over = compare_mappings_tie_aware(oracle, om, reads, mp.arrays(), omp, use_max_ratio=use_max_ratio, **kw)
    lb = mp.read_logp_backward()[1]
    olb = np.array([om.run_sparse_adaptive(r, use_max_ratio).to_full_prob_backward() for r in reads])
    t2 = scores_tie_aware(oracle, lb, olb, lambda b: om.run_sparse_adaptive(reads[b], use_max_ratio).to_full_prob_backward(),
                          tol=TOL_ADAPT)
    print(f"{what}: |d ln P| {_dev(lp, olp):.3e}, |d backward ln P| {_dev(lb, olb):.3e} (bar {TOL_ADAPT:.0e}); reads that needed "
          f"another tie order: scores {t0}, lists {t1}, backward {t2}; overflow {over}")
    if use_max_ratio:
        assert t0 == t1 == t2 == over == 0  # (the CPU test: the oracle's scores do not move under any tie rule)
        _held(what + ", node usage", _dev(nf, onf), TOL_USAGE * len(reads))
    elif t0 + t1 + over == 0:
        _held(what + ", node usage", _dev(nf, onf), TOL_USAGE * len(reads))


@pytest.mark.parametrize("which", ["dbg", "u20"])
def test_sparse_backward_and_run_sparse(gpu_lib, oracle, which):
    f = _fixture(which)
    arrays, reads = f["arrays"], f["reads"]
    gm, om, rc = D.PHMMModel(arrays), oracle.Model(arrays), D.ReadCollection(reads)
    _, lpb = gm.to_full_prob_sparse_backward(rc)
    outs = [om.run_sparse(r) for r in reads]
    olb = np.array([o.to_full_prob_backward() for o in outs])
    olf = np.array([o.to_full_prob_forward() for o in outs])
    t0 = scores_tie_aware(oracle, lpb, olb, lambda b: om.backward(reads[b], oracle.BWD_SPARSE).full_prob(), tol=TOL_ADAPT)
    lf, lb, nf = gm.run_sparse(rc)
    t1 = scores_tie_aware(oracle, lf, olf, lambda b: om.run_sparse(reads[b]).to_full_prob_forward(), tol=TOL_ADAPT)
    t2 = scores_tie_aware(oracle, lb, olb, lambda b: om.run_sparse(reads[b]).to_full_prob_backward(), tol=TOL_ADAPT)
    print(f"{which}(): sparse backward |d ln P| {_dev(lpb, olb):.3e}, run_sparse forward {_dev(lf, olf):.3e} backward "
          f"{_dev(lb, olb):.3e} (bar {TOL_ADAPT:.0e}); tie retries {t0} {t1} {t2}")
    assert np.array_equal(lb, lpb) or _dev(lb, lpb) < TOL_LOGP
    if t0 + t1 + t2 == 0:
        # state_probs = the emit probs summed over the merged indices (freq.rs:236-243), as tests/test_gpu_sparse.py sums them
        onf = np.zeros(arrays.n_nodes)
        for o, r in zip(outs, reads):
            for jj in range(len(r) + 1):
                m, i, d, _ = o.to_emit_probs(jj)
                with np.errstate(under="ignore"):
                    onf += np.exp(m) + np.exp(i) + np.exp(d)
        _held(f"{which}(), run_sparse node usage", _dev(nf, onf), TOL_USAGE * len(reads))


# ------------------------------------------------------------------ 5. the list passes
_REFS = {}


def _list_refs(oracle, which, width):
    """the oracle's results of the four list calls on one set of lists; computed once, shared, left unchanged"""
    key = (which, width)
    if key not in _REFS:
        f = _fixture(which)
        arrays, reads = f["arrays"], f["reads"]
        po, nd = _lists(which, width)
        om = oracle.Model(arrays)

        class _RC:
            offsets = P.offsets(reads)
        arr = (po, nd, np.zeros(nd.size))
        (kpo, knd, klp), knf = om.generate_mappings(reads, arr, True, n_threads=8)
        lb = np.array([om.run_with_mapping(r, oracle.Mapping(*subset_csr(_RC.offsets, arr, [i]))).to_full_prob_backward()
                       for i, r in enumerate(reads)])
        _REFS[key] = dict(po=po, nd=nd, kept=(kpo, knd, klp), nf=knf, lb=lb, edges=_oracle_sums(oracle, arrays, reads, _RC, arr),
                          states=oracle_states(oracle, arrays, reads, _RC, (po, nd)), tables=oracle_tables(oracle, arrays, reads, po, nd))
    return _REFS[key]


def _hold_entries(what, po, got, ref):
    """state posteriors, [entries, 3]: at or above ln 1e-12 held at 1e-8, below it under the floor on the GPU too"""
    hi = ref >= LN_FLOOR
    assert got.shape == ref.shape and not np.any(np.isnan(got))
    with np.errstate(invalid="ignore"):
        d = float(np.max(np.abs(got[hi] - ref[hi])))
    assert np.all(got[~hi] < LN_FLOOR + TOL_ENTRY), what
    _held(what, d, TOL_ENTRY)


def _hold_list_tables(what, po, got, ref):
    po = po.astype(np.int64)
    worst = 0.0
    for ent, scal in (("f", "fs"), ("b", "bs")):
        for g in range(po.size - 1):
            e = slice(int(po[g]), int(po[g + 1]))
            worst = max(worst, _hold_log_table(f"{what}, {ent} position {g}", np.concatenate([got[ent][e].reshape(-1), got[scal][g]]),
                                               np.concatenate([ref[ent][e].reshape(-1), ref[scal][g]])))
    _held(what + ", table entries and scalars", worst, TOL_ENTRY)
    _held(what + ", table totals", max(_dev(got["lf"], ref["lf"]), _dev(got["lb"], ref["lb"])), TOL_LOGP)


def _list_passes(oracle, which, width, what, want_block=None):
    f = _fixture(which)
    arrays, reads = f["arrays"], f["reads"]
    ref = _list_refs(oracle, which, width)
    po, nd = ref["po"], ref["nd"]
    n = len(reads)
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    mp = D.Mappings.from_arrays(rc, po, nd)
    block = {}
    # generate_mappings with the lists given (hint.rs:199-219)
    kept, nf = gm.generate_mappings(rc, mp, True)
    block["lists"] = _ffi.last_call_stats(STATS_WIDE)[1]
    _held(what + ", lists call, forward ln P", _dev(kept.read_logp()[1], ref["edges"][0]), TOL_LOGP)
    _held(what + ", lists call, backward ln P", _dev(kept.read_logp_backward()[1], ref["lb"]), TOL_LOGP)
    compare_mappings(reads, kept.arrays(), ref["kept"], ratio=arrays.param.active_node_max_ratio)
    _held(what + f", lists call, node usage over {n} reads", _dev(nf, ref["nf"]), TOL_USAGE * n)
    # run_with_mapping_edge_freqs
    lf, ef, inf = gm.run_with_mapping_edge_freqs(rc, mp)
    block["edges"] = _ffi.last_call_stats(STATS_WIDE)[1]
    _held(what + ", edges call, ln P", _dev(lf, ref["edges"][0]), TOL_LOGP)
    _held(what + f", edge and init frequencies over {n} reads", max(_dev(ef, ref["edges"][1]), _dev(inf, ref["edges"][2])), TOL_FREQ * n)
    # run_with_mapping_states
    lf, sl, best = gm.run_with_mapping_states(rc, mp)
    block["states"] = _ffi.last_call_stats(STATS_WIDE)[1]
    _held(what + ", states call, ln P", _dev(lf, ref["states"][0]), TOL_LOGP)
    _hold_entries(what + ", state posteriors", po, sl, ref["states"][1])
    # run_with_mapping_tables
    t = gm.run_with_mapping_tables(rc, mp)
    _hold_list_tables(what, po, {"lf": t.logp_forward, "lb": t.logp_backward, "f": t.fwd, "fs": t.fwd_scal, "b": t.bwd,
                                 "bs": t.bwd_scal}, ref["tables"])
    print(f"{what}: block launches {block}")
    if want_block is not None:
        assert all((v > 0) == want_block for v in block.values()), block
    return block


@pytest.mark.parametrize("width", [None, 64, 65, 400], ids=["as_generated", "pad64", "pad65", "pad400"])
def test_list_passes_dbg(gpu_lib, oracle, width):
    _list_passes(oracle, "dbg", width, f"dbg(), lists {'as generated' if width is None else 'padded to %d' % width}")


FLAVOURS = {"generic": {"PHMM_NO_WIDE_HINTED": "1"}, "block_forward": {"PHMM_WIDE_HINTED": "1"},
            "block_edge_backward": {"PHMM_WIDE_HINTED": "1", "PHMM_WIDE_EDGE_BWD": "1"},
            "block_states_backward": {"PHMM_WIDE_HINTED": "1", "PHMM_WIDE_STATES_BWD": "1"},
            "block_of_128": {"PHMM_WIDE_HINTED": "1", "PHMM_WIDE_BWD_T": "128"}}


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_list_passes_u20(gpu_lib, oracle, monkeypatch, flavour):
    """the generic kernels, then the block flavours; phmm_last_call_stats(4, ..) shows that the block ran"""
    for k, v in FLAVOURS[flavour].items():
        monkeypatch.setenv(k, v)
    _list_passes(oracle, "u20", None, f"u20(), {flavour}", want_block=flavour != "generic")


# ------------------------------------------------------------------ 6. the walks
WALK_WIDTHS = pytest.mark.parametrize("width", [None, 65, 400], ids=["as_generated", "pad65", "pad400"])


@WALK_WIDTHS
def test_best_path_and_its_alignments(gpu_lib, oracle, width):
    arrays, reads, po, nd = P.walk_case(width)
    gm, rc, om = D.PHMMModel(arrays), D.ReadCollection(reads), oracle.Model(arrays)
    mp = D.Mappings.from_arrays(rc, po, nd)
    lp, path, counts = gm.run_with_mapping_best_path(rc, mp)
    off = rc.offsets.astype(np.int64)
    lists = [_read_lists(po, nd, off, j) for j in range(len(reads))]
    for j, r in enumerate(reads):
        B.check_read(arrays, r, lists[j], float(lp[j]), path[off[j]:off[j + 1]], counts[j].tolist())
        assert lp[j] <= om.forward_score_only(r, oracle.Mapping.from_lists(lists[j])) + TOL_LOGP
    assert np.all(np.isfinite(lp))
    # the records of the same walks
    alp, _, acounts, al = gm.run_with_mapping_alignments(rc, mp)
    assert np.array_equal(alp, lp) and np.array_equal(acounts[:, 0, :], counts)
    arr = al.arrays()
    for j, r in enumerate(reads):
        rows = path[off[j]:off[j + 1]]
        rec = A.records_of(arr, al.index(j, 0))
        assert rec == A.compress(arrays, r, lists[j], rows), j
        A.check_invariants(*rec, len(r), counts[j].tolist())
        assert al.states(al.index(j, 0)) == A.states_of_rows(lists[j], rows)
    print(f"best path, {len(reads)} reads, longest list {int(np.diff(po.astype(np.int64)).max())}: ln P, rows, counts and records "
          f"equal the restatement's word for word; ln P {lp}")


@WALK_WIDTHS
def test_weighted_walk_and_mea(gpu_lib, oracle, width):
    arrays, reads, po, nd = P.walk_case(width)
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    mp = D.Mappings.from_arrays(rc, po, nd)
    off = rc.offsets.astype(np.int64)
    rng = np.random.default_rng([20261021, 0 if width is None else width])
    w = rng.normal(size=(int(po[-1]), 3)) * 10.0 ** rng.integers(-2, 3, size=(int(po[-1]), 3))
    ib = rng.normal(size=int(off[-1]))
    score, path, counts = gm.run_with_mapping_weighted_path(rc, mp, w, ib)

    def hold(w, ib, score, path, counts):
        for j, r in enumerate(reads):
            e0, e1 = int(po[off[j]]), int(po[off[j + 1]])
            want = M.check_read(arrays, r, _read_lists(po, nd, off, j), w[e0:e1], None if ib is None else ib[off[j]:off[j + 1]],
                                float(score[j]), path[off[j]:off[j + 1]], counts[j].tolist())
            assert want > NINF
    hold(w, ib, score, path, counts)
    # MEA: the states call's posteriors as weights (held to the oracle in the list passes), then the same walk
    lf, score, path, counts, mw = gm.run_with_mapping_mea_path(rc, mp, 1.0, want_weights=True)
    lf_s, sl, _ = gm.run_with_mapping_states(rc, mp, want_best=False)
    assert np.array_equal(lf, lf_s)
    with np.errstate(under="ignore"):
        want_w = np.exp(sl)
    normal = want_w >= 2.0 ** -1022
    assert np.all(np.abs(mw - want_w)[normal] <= 4.0 * 2.0 ** -52 * want_w[normal]) and np.all(np.abs(mw - want_w)[~normal] <= 4.0 * 2.0 ** -1074)
    hold(mw, None, score, path, counts)
    print(f"weighted walk and MEA, {len(reads)} reads, longest list {int(np.diff(po.astype(np.int64)).max())}: scores, rows and "
          f"counts equal the restatement's word for word; MEA scores {score}")


@WALK_WIDTHS
def test_sample_paths_and_their_alignments(gpu_lib, oracle, width):
    """4 samples per read; tests/test_distinct_params_cpu.py asserts that no decision of these walks has a margin below
    1e-9 (a condition on the inputs: the device's exp and Python's may differ in the last bits)"""
    arrays, reads, po, nd = P.walk_case(width)
    gm, rc, om = D.PHMMModel(arrays), D.ReadCollection(reads), oracle.Model(arrays)
    mp = D.Mappings.from_arrays(rc, po, nd)
    off = rc.offsets.astype(np.int64)
    lists = [_read_lists(po, nd, off, j) for j in range(len(reads))]
    want = S.sample_set(arrays, reads, lists, 4, P.SAMPLE_SEED)
    lp, plp, path, counts, usage = gm.run_with_mapping_sample_paths(rc, mp, 4, P.SAMPLE_SEED, want_usage=True)
    worst_z = worst_p = 0.0
    for j, (r, ls) in enumerate(zip(reads, lists)):
        total = om.forward_score_only(r, oracle.Mapping.from_lists(ls))
        worst_z = max(worst_z, abs(lp[j] - total))
        for s in range(4):
            rows = path[s, off[j]:off[j + 1]]
            if not np.array_equal(rows, want[j]["rows"][s]):
                raise AssertionError(S.first_difference(arrays, r, ls, j, s, P.SAMPLE_SEED, rows))
            v, n_terms, cnt = S.score_path(arrays, r, ls, rows)
            assert cnt == counts[j, s].tolist()
            worst_p = max(worst_p, abs(plp[j, s] - (v + want[j]["corr"][s])) / S.bar(n_terms, v))
    _held("sample paths, ln Z against forward_score_only", worst_z, TOL_LOGP)
    _held("sample paths, path ln P against the re-scored rows, in bars", worst_p, 1.0)
    for s in range(4):
        assert np.array_equal(usage[s], S.usage_of(path[s], reads, lists, arrays.n_nodes)), s
    alp, aplp, acounts, al = gm.run_with_mapping_alignments(rc, mp, 4, P.SAMPLE_SEED)
    assert np.array_equal(alp, lp) and np.array_equal(aplp, plp) and np.array_equal(acounts, counts)
    arr = al.arrays()
    for j, r in enumerate(reads):
        for s in range(4):
            rec = A.records_of(arr, al.index(j, s))
            assert rec == A.compress(arrays, r, lists[j], want[j]["rows"][s]), (j, s)
            A.check_invariants(*rec, len(r), counts[j, s].tolist())
    print(f"sample paths, {len(reads)} reads x 4, longest list {int(np.diff(po.astype(np.int64)).max())}: rows, counts, usage and "
          f"records equal the restatement's word for word")


# ------------------------------------------------------------------ 7. reads drawn from the model
GEN_SEED, GEN_WALKS, GEN_LENGTH = P.GEN_SEED, P.GEN_WALKS, P.GEN_LENGTH


def test_sample_reads_word_for_word(gpu_lib):
    """64 walks of 100 states on dbg()'s model, with history (margins: tests/test_distinct_params_cpu.py)"""
    arrays = P.dbg()["arrays"]
    gm = D.PHMMModel(arrays)
    bases, ln, fl, hist, hl, use = gm.sample_reads_raw(0, GEN_WALKS, GEN_LENGTH, "state_count", None, GEN_SEED, True, True)
    want = [G.walk(arrays, GEN_SEED, w, GEN_LENGTH, G.STATE_COUNT, None) for w in range(GEN_WALKS)]
    for w, (b, h, flags, _) in enumerate(want):
        if hist[w, :len(h)].tolist() != h or hl[w] != len(h):
            raise AssertionError(G.first_difference(arrays, GEN_SEED, w, GEN_LENGTH, G.STATE_COUNT, None, hist[w]))
        assert ln[w] == len(b) and bases[w, :len(b)].tobytes() == b and fl[w] == flags, w
    assert np.array_equal(use, G.usage_of([h for _, h, _, _ in want], gm.n_nodes))
    kinds = {k: sum(1 for _, h, _, _ in want for x in h if x not in (G.INS_BEGIN, G.END, G.NONE) and (x & 3) == k) for k in (0, 1, 2)}
    print(f"{GEN_WALKS} walks of {GEN_LENGTH} states equal the restatement's word for word: Match, Ins, Del states {kinds}")
    assert min(kinds.values()) > 0


def test_sample_reads_chi_square(gpu_lib):
    """the 40 000-walk chi-square of tests/test_gpu_sample_reads.py on its small model under DISTINCT"""
    arrays, length, kind = G.chi_case()
    arrays = P.with_param(arrays, P.params(16))
    law = G.exact_law(arrays, length, kind)
    gm = D.PHMMModel(arrays)
    bases, ln, fl, hist, hl, _ = gm.sample_reads_raw(0, G.CHI_WALKS, length, "state_count", None, G.CHI_SEED, True)
    outcomes = [(tuple(hist[w, :hl[w]].tolist()), bases[w, :ln[w]].tobytes()) for w in range(G.CHI_WALKS)]
    chi, df = G.chi_square(law, outcomes)
    print(f"{len(law)} outcomes, chi-square {chi:.1f} at df {df}, bar {G.chi_bar(df):.1f}")
    assert df >= 50 and chi <= G.chi_bar(df)
