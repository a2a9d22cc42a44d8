"""GPU: the HIP path does not depend on how nodes are numbered or edges are ordered, and is right on graphs that are
not DBGs.  dbg_from_haplotypes numbers nodes along unitigs and lists edges by source; 93 % of the nodes of such a model
carry the chain flag (model.cpp) and the dense kernels slide a register window over them, so the general gather path,
the starts of runs and the edge-id mapping are only ever met where the builder puts them.  The ABI promises no order
("edges in petgraph insertion order").  Every case here is one of graph_cases.py's orderings of the DBG
(N = 788), or the zoo graph (self-loop, parallel edge, 7-arm hub, interior `n` node, back edge, unnormalised rows; with
the hub the generic frontier kernels run, without it the one-lane-per-node ones) under `random` and `blocks`, and is
compared two ways:

  parity       with the oracle on the same relabelled arrays;
  invariance   with the GPU's own result on the as-built arrays, carried through the permutation.

Tolerances are the ones the suite already uses for the same quantity (named where they are used); invariance gets the
parity tolerance, not a tighter one: sums in the scaled linear domain change order with the labels.  The oracle itself
is label-independent to 1e-12 (tests/test_relabel_cpu.py).  No read of these cases is a forced switch
(PHMM_READ_FORCED_SWITCH, outside the parity domain): asserted after every adaptive call, under every labelling.
Tie-order retries (helpers.compare_mappings_tie_aware / scores_tie_aware) are counted, printed, and bounded by 1 read
in 8 per comparison.

One test function per entry-point group, so that a failure names its path: `identity` (edge order alone) separates
edge-id defects from node-run defects, `shift3` alignment defects from gather-path defects."""
import functools

import numpy as np
import pytest

import dbgphmm_amd as D
from dbgphmm_amd import _ffi
import graph_cases as G
from helpers import compare_mappings, compare_mappings_tie_aware, finite_close, scores_tie_aware

pytestmark = pytest.mark.gpu

CASES = [("dbg", o) for o in G.ORDERINGS] + [(g, o) for g in ("zoo", "zoo_lean") for o in ("random", "blocks")]
TOL_LOGP = 1e-9    # dense ln P per read (test_gpu_dense.py)
TOL_TABLE = 1e-9   # dense table entries, log space, with the floor of test_tables_match_oracle
TOL_FREQ = 1e-9    # node usage / edge / init frequencies, times the number of reads (test_gpu_dense.py, test_gpu_hinted_edges.py)
TOL_SPARSE = 1e-6  # adaptive-sparse ln P and list node usage per read (fuzz_cases.check_case, test_gpu_sparse.py)
TOL_HINT = 1e-9    # hinted ln P, candidates, change form, handle (fuzz_cases.check_case, test_gpu_copy_num_changes.py)
FORCED = _ffi.PHMM_READ_FORCED_SWITCH


class _Case:
    def __init__(self, graph, ordering):
        self.graph, self.ordering = graph, ordering
        self.base, self.rel = G.base_case(graph), G.relabelled_case(graph, ordering)
        self.reads = self.base["reads"]
        self.npm, self.epm = self.rel["node_perm"], self.rel["edge_perm"]
        self.arrays, self.sg = self.rel["arrays"], self.rel["sg"]
        self.ref, self.ref0 = G.oracle_reference(graph, ordering), G.oracle_reference(graph)
        self.R = len(self.reads)
        self.max_ties = self.R // 8


@pytest.fixture(params=CASES, ids=[f"{g}-{o}" for g, o in CASES])
def case(request, gpu_lib, oracle):
    return _Case(*request.param)


def _dev(a, b):
    return float(np.max(np.abs(np.asarray(a, float) - np.asarray(b, float)), initial=0.0))


def _close(a, b, tol):
    """both -inf, or within tol"""
    a, b = np.asarray(a, float), np.asarray(b, float)
    with np.errstate(invalid="ignore"):
        return bool(np.all((np.isneginf(a) & np.isneginf(b)) | (np.abs(a - b) <= tol)))


def _cut_tol(base_lp, lp):
    """per-read tolerance of a hinted score under a candidate: a read the candidate cuts (more than 100 nats below its
    score under the base vector) is held to 1e-6, the others to 1e-9
    (test_gpu_copy_num_changes.py::test_change_form_matches_full_form)"""
    with np.errstate(invalid="ignore"):
        return np.where(np.asarray(base_lp) - np.asarray(lp) > 100.0, 1e-6, TOL_HINT)


def _same_scores(lp, want, tot, want_tot, base_lp):
    """per-read values within _cut_tol, and the total within the sum of the per-read tolerances"""
    tol = _cut_tol(base_lp, want)
    return _close(lp, want, tol) and _close(tot, want_tot, float(np.sum(tol)))


def _no_forced(rc, what):
    flags = rc.last_call_info()[1]
    assert not np.any(flags & FORCED), (what, "forced-switch read: pick another read seed", flags)


# ---------------------------------------------------------------- dense

def _run_dense(arrays, reads, gaps):
    lf, lb, nf = D.PHMMModel(G.with_gaps(arrays, gaps)).run_dense(D.ReadCollection(reads))
    return dict(lf=lf, lb=lb, nf=nf)


@functools.lru_cache(maxsize=None)
def _dense_as_built(graph, gaps):
    return _run_dense(G.base_case(graph)["arrays"], G.base_case(graph)["reads"], gaps)


@pytest.mark.parametrize("gaps", [0, 4, 5])
def test_dense(case, gaps):
    """run_dense: n_max_gaps = 4 is the last value with the chain window (hop entries), 5 the first without (merged
    closure entries), 0 the shortest closure"""
    c = case
    g = _run_dense(c.arrays, c.reads, gaps)
    olf, olb, onf = G.oracle_dense(c.graph, c.ordering, gaps)
    b = _dense_as_built(c.graph, gaps)
    dev = dict(parity_lf=_dev(g["lf"], olf), parity_lb=_dev(g["lb"], olb), parity_nf=_dev(g["nf"], onf),
               inv_lf=_dev(g["lf"], b["lf"]), inv_lb=_dev(g["lb"], b["lb"]), inv_nf=_dev(g["nf"][c.npm], b["nf"]))
    print(c.graph, c.ordering, gaps, dev)
    assert dev["parity_lf"] < TOL_LOGP and dev["parity_lb"] < TOL_LOGP and dev["parity_nf"] < TOL_FREQ * c.R, dev
    assert dev["inv_lf"] < TOL_LOGP and dev["inv_lb"] < TOL_LOGP and dev["inv_nf"] < TOL_FREQ * c.R, dev


def test_dense_full_width(case):
    """128 reads (the 12, ten times, and the first 8 again): the 64-reads-per-wave instantiation of the dense kernels
    (rows fetched through LDS, uniform node ids), which 12 reads never reach"""
    c = case
    many = c.reads * 10 + c.reads[:8]
    lf, lb, nf = D.PHMMModel(c.arrays).run_dense(D.ReadCollection(many))
    olf, olb, onf = G.oracle_dense(c.graph, c.ordering, 4)
    _, _, onf8 = c.ref["model"].run_dense_reads(c.reads[:8], n_threads=8)
    want_lf, want_lb = np.concatenate([np.tile(olf, 10), olf[:8]]), np.concatenate([np.tile(olb, 10), olb[:8]])
    dev = dict(lf=_dev(lf, want_lf), lb=_dev(lb, want_lb), nf=_dev(nf, 10 * onf + onf8))
    print(c.graph, c.ordering, dev)
    assert dev["lf"] < TOL_LOGP and dev["lb"] < TOL_LOGP and dev["nf"] < TOL_FREQ * len(many), dev


def _two_reads(reads):
    return [reads[1], reads[6][:40]]


def _run_tables(arrays, reads):
    gm = D.PHMMModel(arrays)
    return [(gm.forward(r), gm.backward(r)) for r in _two_reads(reads)]


@functools.lru_cache(maxsize=None)
def _tables_as_built(graph):
    return _run_tables(G.base_case(graph)["arrays"], G.base_case(graph)["reads"])


def test_dense_tables(case):
    """phmm_dense_tables of two reads: all six tables against the oracle's, and against the as-built GPU tables with
    the columns permuted"""
    c = case
    got, base = _run_tables(c.arrays, c.reads), _tables_as_built(c.graph)
    om = c.ref["model"]
    for read, (f, b), (f0, b0) in zip(_two_reads(c.reads), got, base):
        of, ob = om.forward(read), om.backward(read)
        for i in range(len(read)):
            for name, t, t0, o in (("F", f, f0, of), ("B", b, b0, ob)):
                m, ins, d, s = o.table(i)
                floor = max(m.max(), ins.max(), d.max()) - 600.0
                for w, mine, ref, theirs in (("m", t.m[i], m, t0.m[i]), ("i", t.i[i], ins, t0.i[i]), ("d", t.d[i], d, t0.d[i])):
                    assert finite_close(mine, ref, TOL_TABLE, floor).all(), (c.graph, c.ordering, len(read), i, name + w)
                    back = mine[c.npm]  # the value of as-built node v sits at its new id
                    assert (finite_close(back, theirs, TOL_TABLE, floor) | finite_close(theirs, back, TOL_TABLE, floor)).all(), \
                        (c.graph, c.ordering, len(read), i, name + w, "invariance")
                assert finite_close(t.scal[i], s, TOL_TABLE).all(), (c.graph, c.ordering, len(read), i, name + "scal")
                assert finite_close(t.scal[i], t0.scal[i], TOL_TABLE).all(), (c.graph, c.ordering, len(read), i, name + "scal", "invariance")


def _run_edges(arrays, reads):
    gm = D.PHMMModel(arrays)
    lf, ef, inf = gm.run_dense_edge_freqs(D.ReadCollection(reads))
    return dict(lf=lf, ef=ef, inf=inf, q=gm.q_score_exact(ef, inf))


@functools.lru_cache(maxsize=None)
def _edges_as_built(graph):
    return _run_edges(G.base_case(graph)["arrays"], G.base_case(graph)["reads"])


def test_dense_edge_freqs_and_q_score(case):
    """run_dense_edge_freqs: edge_freq is indexed by the caller's edge ids (par_edge / chi_edge -> out_edge_freq), so
    it is compared at [edge_perm], init_freq at [node_perm]; q_score_exact walks the child CSR back to edge ids"""
    c = case
    g, b = _run_edges(c.arrays, c.reads), _edges_as_built(c.graph)
    dev = dict(parity_lf=_dev(g["lf"], c.ref["lf_edges"]), parity_ef=_dev(g["ef"], c.ref["ef"]),
               parity_inf=_dev(g["inf"], c.ref["inf"]), inv_lf=_dev(g["lf"], b["lf"]),
               inv_ef=_dev(g["ef"][c.epm], b["ef"]), inv_inf=_dev(g["inf"][c.npm], b["inf"]))
    print(c.graph, c.ordering, dev, g["q"], b["q"])
    assert dev["parity_lf"] < TOL_LOGP and dev["inv_lf"] < TOL_LOGP, dev
    assert max(dev["parity_ef"], dev["parity_inf"], dev["inv_ef"], dev["inv_inf"]) < TOL_FREQ * c.R, dev
    # q_score_exact: the numpy expression of test_gpu_dense.py::test_q_score_exact on the ORACLE's posteriors
    a = c.arrays
    emit = a.emission != ord("n")
    ok_e = emit[a.edge_src] & emit[a.edge_dst]
    want_init = float(np.sum(c.ref["inf"][emit] * a.init_logp[emit]))
    want_trans = float(np.sum(c.ref["ef"][ok_e] * a.trans_logp[ok_e]))
    qi, qt, qp = g["q"]
    assert qp == 0.0 and qi < 0 and qt <= 0
    assert abs(qi - want_init) < 1e-6 * max(1.0, abs(want_init)), (qi, want_init)
    assert abs(qt - want_trans) < 1e-6 * max(1.0, abs(want_trans)), (qt, want_trans)
    assert abs(qi - b["q"][0]) < 1e-6 * max(1.0, abs(want_init)) and abs(qt - b["q"][1]) < 1e-6 * max(1.0, abs(want_trans))


# ---------------------------------------------------------------- adaptive sparse

def _run_adaptive(arrays, reads):
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    out = {}
    _, out["lp"] = gm.to_full_prob_reads(rc, None, True)
    _no_forced(rc, "to_full_prob_reads")
    mp, out["nf"] = gm.generate_mappings(rc, None, True)
    _no_forced(rc, "generate_mappings")
    out["mp"] = mp.arrays()
    out["mp_lf"], out["mp_lb"] = mp.read_logp()[1], mp.read_logp_backward()[1]
    assert np.array_equal(out["mp_lf"], out["lp"])  # the score flow and the mapping flow: the same forward pass
    return out


@functools.lru_cache(maxsize=None)
def _adaptive_as_built(graph):
    return _run_adaptive(G.base_case(graph)["arrays"], G.base_case(graph)["reads"])


def test_adaptive_sparse(case, oracle):
    """to_full_prob_reads(None, ratio mode), generate_mappings(None, ratio mode) with its lists, node usage and the
    per-read forward / backward totals"""
    c = case
    g, b = _run_adaptive(c.arrays, c.reads), _adaptive_as_built(c.graph)
    om, om0 = c.ref["model"], c.ref0["model"]
    ratio = c.arrays.param.active_node_max_ratio
    dev = dict(parity_lp=_dev(g["lp"], c.ref["lp"]), inv_lp=_dev(g["lp"], b["lp"]),
               parity_nf=_dev(g["nf"], c.ref["mp_nf"]), inv_nf=_dev(g["nf"][c.npm], b["nf"]),
               inv_lb=_dev(g["mp_lb"], b["mp_lb"]))
    assert dev["parity_lp"] < TOL_SPARSE and dev["inv_lp"] < TOL_SPARSE, dev
    # the lists on the new labels against the oracle on the new labels; mapped back, against the as-built oracle's
    t1, o1 = compare_mappings_tie_aware(oracle, om, c.reads, g["mp"], c.ref["mp"], ratio=ratio)
    back = G.carry_mappings(g["mp"], G.inverse(c.npm))
    t2, o2 = compare_mappings_tie_aware(oracle, om0, c.reads, back, c.ref0["mp"], ratio=ratio)
    want_lb = np.array([om.run_sparse_adaptive(r, True).to_full_prob_backward() for r in c.reads])
    t3 = scores_tie_aware(oracle, g["mp_lb"], want_lb, lambda i: om.run_sparse_adaptive(c.reads[i], True).to_full_prob_backward())
    # invariance of the backward totals: a read whose total moved with the labels must hang on the tie order
    i3 = scores_tie_aware(oracle, g["mp_lb"], b["mp_lb"], lambda i: om0.run_sparse_adaptive(c.reads[i], True).to_full_prob_backward())
    print(c.graph, c.ordering, dev, "tie-order reads: lists", t1, "lists mapped back", t2, "backward totals", t3, i3,
          "overflow", o1, o2)
    assert max(t1, t2, t3, i3) <= c.max_ties and o1 == 0 and o2 == 0
    assert dev["parity_nf"] < TOL_SPARSE * c.R and dev["inv_nf"] < TOL_SPARSE * c.R, dev


def _run_topk(arrays, reads):
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    out = {}
    _, out["lpk"] = gm.to_full_prob_reads(rc, None, False)
    mpk, _ = gm.generate_mappings(rc, None, False)
    out["mpk"] = mpk.arrays()
    _, out["lpb"] = gm.to_full_prob_sparse_backward(rc)
    out["lfs"], out["lbs"], out["nfs"] = gm.run_sparse(rc)
    # (fuzz_cases.check_case) run_sparse is the fixed-size forward and the sparse backward
    assert np.array_equal(out["lbs"], out["lpb"]) or _dev(out["lbs"], out["lpb"]) < 1e-9
    assert _dev(out["lfs"], out["lpk"]) < 1e-9
    return out


@functools.lru_cache(maxsize=None)
def _topk_as_built(graph):
    return _run_topk(G.base_case(graph)["arrays"], G.base_case(graph)["reads"])


def test_fixed_size_mode_and_sparse_backward(case, oracle):
    """use_max_ratio = false (top n_active_nodes): scores and lists; to_full_prob_sparse_backward; run_sparse"""
    c = case
    g, b = _run_topk(c.arrays, c.reads), _topk_as_built(c.graph)
    om, om0 = c.ref["model"], c.ref0["model"]
    reads = c.reads
    olpk = om.full_prob_reads(reads, None, False, n_threads=8)
    n_k = scores_tie_aware(oracle, g["lpk"], olpk, lambda i: om.full_prob_reads([reads[i]], None, False, n_threads=1)[0])
    ompk, _ = om.generate_mappings(reads, None, False, n_threads=8)
    t_k, o_k = compare_mappings_tie_aware(oracle, om, reads, g["mpk"], ompk, use_max_ratio=False,
                                          top_k=c.arrays.param.n_active_nodes)
    olpb = np.array([om.backward(r, oracle.BWD_SPARSE).full_prob() for r in reads])
    n_b = scores_tie_aware(oracle, g["lpb"], olpb, lambda i: om.backward(reads[i], oracle.BWD_SPARSE).full_prob())
    # invariance: a read whose score moved with the labels must be one that hangs on the tie order (the as-built
    # oracle gives the relabelled GPU's value under one of the other tie rules)
    i_k = scores_tie_aware(oracle, g["lpk"], b["lpk"], lambda i: om0.full_prob_reads([reads[i]], None, False, n_threads=1)[0])
    i_b = scores_tie_aware(oracle, g["lpb"], b["lpb"], lambda i: om0.backward(reads[i], oracle.BWD_SPARSE).full_prob())
    print(c.graph, c.ordering, "tie-order reads: scores", n_k, "lists", t_k, "sparse backward", n_b, "invariance", i_k, i_b,
          "overflow", o_k, "max |d node usage| against as built", _dev(g["nfs"][c.npm], b["nfs"]))
    assert max(n_k, t_k, n_b, i_k, i_b) <= c.max_ties and o_k == 0
    if not (n_k or t_k or n_b or i_k or i_b):
        # run_sparse's node usage (test_gpu_sparse.py::test_run_sparse_node_freqs_match_oracle: 1e-9 per read)
        assert _dev(g["nfs"][c.npm], b["nfs"]) < 1e-9 * c.R


# ---------------------------------------------------------------- hinted

@functools.lru_cache(maxsize=None)
def _candidates(graph):
    """as-built: (base vector, 4 candidate vectors, their change lists, groups, 4 group candidates) -- every case of
    `graph` carries these same candidates to its labels"""
    b = G.base_case(graph)
    sg = b["sg"]
    rng = np.random.default_rng(17)
    cands = G.copy_num_candidates(sg, G.oracle_reference(graph)["mp"], b["reads"], rng)
    base = cands[0].copy()
    changes = D.model.copy_num_changes(base, cands)
    goff, gnodes = D.unitig_groups(sg)
    n_groups = goff.size - 1
    gbase = base[gnodes[goff[:-1].astype(np.int64)]]
    gc = []
    for _ in range(4):
        gs = rng.choice(n_groups, size=int(rng.integers(1, 4)), replace=False)
        gc.append((gs, np.maximum(gbase[gs].astype(np.int64) + rng.choice([-1, 1], size=gs.size), 0)))
    return base, cands, changes, (goff, gnodes), gc


def _csr(cand_changes):
    off = np.zeros(len(cand_changes) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(n) for n, _ in cand_changes])
    ids = np.concatenate([np.asarray(n, np.uint32) for n, _ in cand_changes] + [np.zeros(0, np.uint32)])
    cn = np.concatenate([np.asarray(v, np.uint32) for _, v in cand_changes] + [np.zeros(0, np.uint32)])
    return off, ids, cn


def _expand(groups, cand_changes):
    goff, gnodes = groups
    goff = goff.astype(np.int64)
    out = []
    for gs, vals in cand_changes:
        nodes = [gnodes[goff[g]:goff[g + 1]] for g in gs]
        cns = [np.full(int(goff[g + 1] - goff[g]), v, np.uint32) for g, v in zip(gs, vals)]
        out.append((np.concatenate(nodes + [np.zeros(0, np.uint32)]), np.concatenate(cns + [np.zeros(0, np.uint32)])))
    return out


def _run_hinted(arrays, reads, hint):
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    gmp = D.Mappings.from_arrays(rc, *hint)
    out = {}
    _, out["lp"] = gm.to_full_prob_reads(rc, gmp)
    mph, out["nf"] = gm.generate_mappings(rc, gmp, True)
    out["mp"], out["mp_lb"] = mph.arrays(), mph.read_logp_backward()[1]
    out["e_lf"], out["ef"], out["inf"] = gm.run_with_mapping_edge_freqs(rc, gmp)
    return out


@functools.lru_cache(maxsize=None)
def _hinted_as_built(graph):
    return _run_hinted(G.base_case(graph)["arrays"], G.base_case(graph)["reads"], G.oracle_reference(graph)["hint"])


def test_hinted(case, oracle):
    """the oracle's as-built lists carried to the new labels: to_full_prob_reads with them, generate_mappings from
    them, run_with_mapping_edge_freqs over them"""
    c = case
    hint = c.ref["hint"]
    g, b = _run_hinted(c.arrays, c.reads, hint), _hinted_as_built(c.graph)
    om = c.ref["model"]
    omph, onf = om.generate_mappings(c.reads, hint, True, n_threads=8)
    olf, olb, oef, oinf = G.oracle_mapping_sums(oracle, c.arrays, c.reads, hint)
    dev = dict(parity_lp=_dev(g["lp"], c.ref["lp_hint"]), inv_lp=_dev(g["lp"], b["lp"]),
               parity_nf=_dev(g["nf"], onf), inv_nf=_dev(g["nf"][c.npm], b["nf"]),
               parity_lb=_dev(g["mp_lb"], olb), inv_lb=_dev(g["mp_lb"], b["mp_lb"]),
               parity_e_lf=_dev(g["e_lf"], olf), inv_e_lf=_dev(g["e_lf"], b["e_lf"]),
               parity_ef=_dev(g["ef"], oef), inv_ef=_dev(g["ef"][c.epm], b["ef"]),
               parity_inf=_dev(g["inf"], oinf), inv_inf=_dev(g["inf"][c.npm], b["inf"]))
    print(c.graph, c.ordering, dev)
    assert dev["parity_lp"] < TOL_HINT and dev["inv_lp"] < TOL_HINT, dev
    ratio = c.arrays.param.active_node_max_ratio
    compare_mappings(c.reads, g["mp"], omph, ratio=ratio)  # (no top-k cut on this way: no tie retry, check_case)
    compare_mappings(c.reads, G.carry_mappings(g["mp"], G.inverse(c.npm)), b["mp"], ratio=ratio)
    assert dev["parity_nf"] < TOL_SPARSE * c.R and dev["inv_nf"] < TOL_SPARSE * c.R, dev
    assert dev["parity_lb"] < TOL_HINT and dev["inv_lb"] < TOL_HINT, dev  # (test_gpu_backward_total.py: hinted, 1e-9)
    tol = TOL_FREQ * c.R  # (test_gpu_hinted_edges.py::_check_oracle: ln P, edge and init frequencies alike)
    assert max(dev["parity_e_lf"], dev["parity_ef"], dev["parity_inf"]) < tol, dev
    assert max(dev["inv_e_lf"], dev["inv_ef"], dev["inv_inf"]) < tol, dev


def _run_candidates(arrays, sg, reads, hint, base, cands, changes):
    """full form and change form of the 4 candidates; rescored reads carry the bits of the full form"""
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    gmp = D.Mappings.from_arrays(rc, *hint)
    tot_f, lp_f = gm.to_full_prob_reads_copy_nums(rc, gmp, cands, 0)
    tot, lp, nres = gm.to_full_prob_reads_copy_num_changes(rc, gmp, base, changes, 0)
    exp = G.expected_rescored(sg, base, changes, 0, reads, hint)
    assert np.array_equal(nres, exp.sum(axis=1)), (nres, exp.sum(axis=1))
    for k in range(cands.shape[0]):
        assert np.array_equal(lp[k][exp[k]], lp_f[k][exp[k]]), k  # rescored pairs: the same bits
        assert _close(lp[k], lp_f[k], TOL_HINT), k
        _, l1 = gm.to_full_prob_reads_copy_nums(rc, gmp, cands[k:k + 1], 0)
        assert np.array_equal(l1[0], lp_f[k]), k  # a candidate alone has the bits it has in the batch
    assert _close(tot, tot_f, TOL_HINT * len(reads))
    return dict(lp_f=lp_f, tot_f=tot_f, lp=lp, tot=tot, nres=nres)


@functools.lru_cache(maxsize=None)
def _candidates_as_built(graph):
    b = G.base_case(graph)
    base, cands, changes, _, _ = _candidates(graph)
    return _run_candidates(b["arrays"], b["sg"], b["reads"], G.oracle_reference(graph)["hint"], base, cands, changes)


def test_copy_num_candidates(case, oracle):
    """to_full_prob_reads_copy_nums with 4 candidate vectors (permuted; the last zeroes a k-mer on read 0's path) and
    to_full_prob_reads_copy_num_changes with the same candidates as carried change lists"""
    c = case
    base0, cands0, changes0, _, _ = _candidates(c.graph)
    base, cands = G.carry_vector(base0, c.npm), G.carry_vector(cands0, c.npm)
    changes = G.carry_changes(changes0, c.npm)
    hint = c.ref["hint"]
    g = _run_candidates(c.arrays, c.sg, c.reads, hint, base, cands, changes)
    b = _candidates_as_built(c.graph)
    # the zeroed k-mer cuts read 0: only the InsBegin chain carries it on
    assert g["lp_f"][3][0] < g["lp_f"][0][0] - 100.0 and np.all(np.isfinite(g["lp_f"][:3]))
    for k in range(4):
        # the oracle on the host-built model of the candidate (seq_graph.rs:160-209), as fuzz_cases.check_case; a read
        # that a candidate cuts (more than 100 nats below the base) is held to 1e-6, the others to 1e-9
        # (test_gpu_copy_num_changes.py::test_change_form_matches_full_form)
        with np.errstate(divide="ignore"):
            ak = D.vectorised_to_phmm(D.SeqGraph(cands[k].astype(np.int64), c.sg.base, c.sg.edge_src, c.sg.edge_dst, None),
                                      c.arrays.param, 0)
        ol = oracle.Model(ak).full_prob_reads(c.reads, hint, True, n_threads=8)
        tol = _cut_tol(g["lp_f"][0], ol)
        print(c.graph, c.ordering, "candidate", k, "parity", _dev(np.nan_to_num(g["lp_f"][k], neginf=0.0), np.nan_to_num(ol, neginf=0.0)),
              "invariance", _dev(np.nan_to_num(g["lp_f"][k], neginf=0.0), np.nan_to_num(b["lp_f"][k], neginf=0.0)), "cut reads", int((tol > TOL_HINT).sum()))
        assert _close(g["lp_f"][k], ol, tol), (k, g["lp_f"][k], ol)
        assert _same_scores(g["lp_f"][k], b["lp_f"][k], g["tot_f"][k], b["tot_f"][k], b["lp_f"][0]), k
        assert _same_scores(g["lp"][k], b["lp"][k], g["tot"][k], b["tot"][k], b["lp_f"][0]), k
    assert np.array_equal(g["nres"], b["nres"])


def _run_likelihood(arrays, sg, reads, hint, base, cands, changes, groups, gcands):
    """score_changes, three moves and current on a handle; score_group_changes and move_groups on a second one with
    groups, against a third without -> what the calls returned"""
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    gmp = D.Mappings.from_arrays(rc, *hint)
    R = len(reads)
    out = {}
    lk = gm.likelihood(rc, gmp, base, 0)
    tot_s, lp_s, n_s = gm.to_full_prob_reads_copy_num_changes(rc, gmp, base, changes, 0)
    tot, lp, nres = lk.score_changes(changes)
    exp = G.expected_rescored(sg, base, changes, 0, reads, hint)
    assert np.array_equal(nres, n_s) and np.array_equal(nres, exp.sum(axis=1))
    for k in range(exp.shape[0]):
        assert np.array_equal(lp[k][exp[k]], lp_s[k][exp[k]]), k
        assert _close(lp[k], lp_s[k], TOL_HINT), k
    assert _close(tot, tot_s, TOL_HINT * R)
    out["base_lp"] = lk.current()[1]
    out["score"] = [(lp[k], tot[k]) for k in range(exp.shape[0])]
    # three moves: candidates 1, 2 and 3 in turn (the third cuts read 0), each against the full form on the new vector
    vec = base.copy()
    off, node, cn = changes
    out["moves"] = []
    for k in (1, 2, 3):
        nodes, vals = node[int(off[k]):int(off[k + 1])], cn[int(off[k]):int(off[k + 1])]
        one = _csr([(nodes, vals)])
        hit = G.expected_rescored(sg, vec, one, 0, reads, hint)[0]
        t, n = lk.move(nodes, vals)
        vec[nodes] = vals
        cur_cn, cur_lp, cur_tot = lk.current()
        tot_f, lp_f = gm.to_full_prob_reads_copy_nums(rc, gmp, vec[None, :], 0)
        assert np.array_equal(cur_cn, vec) and n == int(hit.sum()), (k, n, int(hit.sum()))
        assert np.array_equal(cur_lp[hit], lp_f[0][hit]) and _close(cur_lp, lp_f[0], TOL_HINT), k
        assert (t == cur_tot or (np.isneginf(t) and np.isneginf(cur_tot))) and _close(t, tot_f[0], TOL_HINT * R), k
        out["moves"].append((cur_lp, t))
    # groups: bit for bit the node form on the expanded lists (test_gpu_likelihood_groups.py)
    lk_g, lk_n = gm.likelihood(rc, gmp, base, 0), gm.likelihood(rc, gmp, base, 0)
    goff, gnodes = groups
    lk_g.set_groups(goff, gnodes)
    gbase = base[gnodes[goff[:-1].astype(np.int64)]]
    assert np.array_equal(lk_g.current_groups(), gbase)
    tot_g, lp_g, n_g = lk_g.score_group_changes(_csr(gcands))
    tot_n, lp_n, n_n = lk_n.score_changes(_csr(_expand(groups, gcands)))
    assert np.array_equal(n_g, n_n) and np.array_equal(lp_g, lp_n) and np.array_equal(tot_g, tot_n)
    out["group_score"] = [(lp_g[k], tot_g[k]) for k in range(len(gcands))]
    gs, vals = gcands[0]
    (nodes, nvals), = _expand(groups, [gcands[0]])
    tg, ng = lk_g.move_groups(gs, vals)
    tn, nn = lk_n.move(nodes, nvals)
    assert tg == tn and ng == nn and ng == n_g[0]
    gvec = gbase.copy()
    gvec[gs] = vals
    assert np.array_equal(lk_g.current_groups(), gvec)
    cg, vg, t_g = lk_g.current()
    cn_, vn, t_n = lk_n.current()
    assert np.array_equal(cg, cn_) and np.array_equal(vg, vn) and t_g == t_n
    out["group_move"] = [(vg, tg)]
    return out


@functools.lru_cache(maxsize=None)
def _likelihood_as_built(graph):
    b = G.base_case(graph)
    return _run_likelihood(b["arrays"], b["sg"], b["reads"], G.oracle_reference(graph)["hint"], *_candidates(graph))


def test_likelihood_handle(case):
    """a Likelihood handle on the new labels: score_changes, three moves, current; after set_groups from the as-built
    unitig groups carried over -- on these labels a group is no run of consecutive ids -- score_group_changes and
    move_groups"""
    c = case
    base0, cands0, changes0, groups0, gcands = _candidates(c.graph)
    g = _run_likelihood(c.arrays, c.sg, c.reads, c.ref["hint"], G.carry_vector(base0, c.npm),
                        G.carry_vector(cands0, c.npm), G.carry_changes(changes0, c.npm),
                        G.carry_groups(groups0, c.npm), gcands)
    b = _likelihood_as_built(c.graph)
    assert _close(g["base_lp"], b["base_lp"], TOL_HINT)
    for what in ("score", "moves", "group_score", "group_move"):
        for j, ((lp, tot), (lp0, tot0)) in enumerate(zip(g[what], b[what])):
            print(c.graph, c.ordering, what, j, "max |d ln P| against as built",
                  _dev(np.nan_to_num(lp, neginf=0.0), np.nan_to_num(lp0, neginf=0.0)), "totals", float(tot), float(tot0))
            assert _same_scores(lp, lp0, tot, tot0, b["base_lp"]), (what, j)


@pytest.mark.parametrize("ordering", G.ORDERINGS)
def test_map_nodes_to_a_relabelled_kp1_graph(gpu_lib, oracle, ordering):
    """Mappings.map_nodes with the node map of hint_kp1_from_hint_k (graph.kp1_node_map) from the relabelled k graph
    into a k+1 graph relabelled on its own: against oracle.map_nodes on the same CSRs, and, mapped back, against the
    GPU on the as-built pair"""
    sg_k1, mo, mn, sg_k = D.graph.kp1_node_map(G.dbg_haplotypes(), G.K)
    b = G.base_case("dbg")
    assert np.array_equal(sg_k.edge_src, b["sg"].edge_src) and np.array_equal(sg_k.base, b["sg"].base)
    c = _Case("dbg", ordering)
    a_k1 = D.vectorised_to_phmm(sg_k1, b["arrays"].param.with_(n_warmup=G.K + 1), 1)
    npm1, epm1 = G.orderings(a_k1, np.random.default_rng(23))[ordering]
    rc = D.ReadCollection(c.reads)
    hint = c.ref["hint"]
    mo2, mn2 = G.carry_node_map(mo, mn, c.npm, npm1)
    gm1, gm1_0 = D.PHMMModel(G.relabel(a_k1, npm1, epm1)), D.PHMMModel(a_k1)
    mp_k, mp_k0 = D.Mappings.from_arrays(rc, *hint), D.Mappings.from_arrays(rc, *c.ref0["hint"])
    got = mp_k.map_nodes(gm1, mo2, mn2).arrays()
    exp = oracle.map_nodes(hint, mo2, mn2)
    base = mp_k0.map_nodes(gm1_0, mo, mn).arrays()
    back = G.carry_mappings(got, G.inverse(npm1))
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[0], base[0])
    for i in range(len(exp[0]) - 1):
        s0, s1 = int(exp[0][i]), int(exp[0][i + 1])
        # (test_gpu_sparse.py::test_mappings_map_nodes_matches_oracle: 1e-9, members as sets)
        assert np.max(np.abs(got[2][s0:s1] - exp[2][s0:s1]), initial=0.0) < 1e-9, i
        assert sorted(got[1][s0:s1].tolist()) == sorted(exp[1][s0:s1].tolist()), i
        assert np.max(np.abs(got[2][s0:s1] - base[2][s0:s1]), initial=0.0) < 1e-9, i
        assert sorted(back[1][s0:s1].tolist()) == sorted(base[1][s0:s1].tolist()), i


# ---------------------------------------------------------------- refusals stay

def test_a_ninth_arm_is_still_refused_on_the_hinted_path(gpu_lib):
    """the zoo graph with 9 arms, relabelled: degree 9 is past what the hinted kernels take (PHMM_EINVAL), however the
    nodes are numbered"""
    sg = G.zoo_graph(arms=9)
    arrays = G.zoo_model(sg)
    npm, epm = G.orderings(arrays, np.random.default_rng(3))["random"]
    reads = G.base_case("zoo")["reads"][:2]
    for a in (arrays, G.relabel(arrays, npm, epm)):
        gm, rc = D.PHMMModel(a), D.ReadCollection(reads)
        T = int(rc.offsets[-1])
        mp = D.Mappings.from_arrays(rc, np.arange(T + 1, dtype=np.uint64), np.zeros(T, np.uint32), np.zeros(T))
        with pytest.raises(D.PhmmError) as e:
            gm.to_full_prob_reads(rc, mp)
        assert e.value.code == _ffi.PHMM_EINVAL
        with pytest.raises(D.PhmmError) as e:
            gm.to_full_prob_reads_copy_nums(rc, mp, np.ones((1, a.n_nodes), np.uint32), 0)
        assert e.value.code == _ffi.PHMM_EINVAL
