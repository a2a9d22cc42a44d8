"""GPU: node groups on the phmm_likelihood handle.  The sampler's state is a copy-number vector over compact edges
(UpdateInfo::cycle(), neighbors.rs:193-216; set_copy_nums, multi_dbg.rs:1041-1052); score_group_changes / move_groups
take it in those units and are, bit for bit, score_changes / move on the change lists expanded to nodes: the same
[C][R] values, totals and rescored counts, and after every move of a chain the same vector, per-read values and total.
The small diploid and the numpy restatement of the rescored set are those of test_gpu_likelihood.py (restated: a test
module cannot be imported without editing it); the groups are graph.unitig_groups of that graph.

Wall time of this file on an MI355X: 5.4 s for its 8 tests (0.6 s of it the module fixture, 1.8 s each chain of 30
moves)."""
import ctypes as C

import numpy as np
import pytest

import dbgphmm_amd as D
from dbgphmm_amd import _ffi

pytestmark = pytest.mark.gpu
K = 20
MIXED = _ffi.PHMM_GROUP_MIXED


def _close(a, b, tol):
    a, b = np.asarray(a, float), np.asarray(b, float)
    both_inf = np.isneginf(a) & np.isneginf(b)
    with np.errstate(invalid="ignore"):
        return bool(np.all(both_inf | (np.abs(a - b) <= tol)))


def _csr(cand_changes):
    """[(ids, new cns)] per candidate -> (off, id, cn)"""
    off = np.zeros(len(cand_changes) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(n) for n, _ in cand_changes])
    ids = np.concatenate([np.asarray(n, np.uint32) for n, _ in cand_changes] + [np.zeros(0, np.uint32)])
    cn = np.concatenate([np.asarray(v, np.uint32) for _, v in cand_changes] + [np.zeros(0, np.uint32)])
    return off, ids, cn


def _expand(groups, cand_changes):
    """group changes [(groups, cns)] -> node changes [(nodes, cns)]: (g, cn) means (v, cn) for every node v of g"""
    goff, gnodes = groups
    out = []
    for gs, vals in cand_changes:
        nodes = [gnodes[goff[g]:goff[g + 1]] for g in gs]
        cns = [np.full(int(goff[g + 1] - goff[g]), v, np.uint32) for g, v in zip(gs, vals)]
        out.append((np.concatenate(nodes + [np.zeros(0, np.uint32)]), np.concatenate(cns + [np.zeros(0, np.uint32)])))
    return out


def _expected_rescored(sg, base, changes, min_cn, rc, mp_arrays):
    """per candidate (node units): non-empty reads whose lists meet A_c = D_c + parents(D_c); all non-empty reads when
    T_c or T_base is 0"""
    po, nd, _ = mp_arrays
    off_r = rc.offsets.astype(np.int64)
    e_lo, e_hi = po[off_r[:-1]].astype(np.int64), po[off_r[1:]].astype(np.int64)
    nonempty = off_r[1:] > off_r[:-1]
    emittable = sg.base != D.graph.NULL_BASE
    eb = np.maximum(base.astype(np.int64), min_cn)
    tb = int(eb[emittable].sum())
    off, node, cn = changes
    out = []
    for c in range(off.size - 1):
        v, k = node[off[c]:off[c + 1]].astype(np.int64), cn[off[c]:off[c + 1]].astype(np.int64)
        ec = eb.copy()
        ec[v] = np.maximum(k, min_cn)
        dc = np.flatnonzero(ec != eb)
        if tb == 0 or int(ec[emittable].sum()) == 0:
            out.append(nonempty.copy())
            continue
        a = np.zeros(base.size, bool)
        a[dc] = True
        a[sg.edge_src[np.isin(sg.edge_dst, dc)]] = True
        hit_e = a[nd].astype(np.int64)
        cum = np.concatenate([[0], np.cumsum(hit_e)])
        out.append(nonempty & (cum[e_hi] > cum[e_lo]))
    return np.array(out)


class _World:
    pass


@pytest.fixture(scope="module")
def world():
    w = _World()
    hap = D.random_genome(12000, seed=11)
    haps = [hap, D.diverge(hap, 0.01, seed=12)]
    w.sg, w.occ = D.dbg_from_haplotypes(haps, K, with_occurrences=True)
    w.param = D.PHMMParams.uniform(0.001).with_(n_warmup=K)
    a1 = D.vectorised_to_phmm(w.sg, w.param, 1)
    w.reads = D.sample_reads(a1, 10 ** 9, 1000, seed=13, max_reads=240)
    w.rc = D.ReadCollection(w.reads)
    w.mp, _ = D.PHMMModel(a1).generate_mappings(w.rc, None, True)
    w.base = w.sg.copy_num.astype(np.uint32)
    goff, gnodes = D.unitig_groups(w.sg)
    w.groups = (goff.astype(np.int64), gnodes)
    w.G = goff.size - 1
    w.group_of = np.empty(w.base.size, np.int64)
    w.group_of[gnodes] = np.repeat(np.arange(w.G), np.diff(w.groups[0]))
    w.gbase = w.base[gnodes[w.groups[0][:-1]]]
    w.models = {mc: D.PHMMModel(D.vectorised_to_phmm(w.sg, w.param, mc)) for mc in (0, 1)}
    return w


def _handles(w, min_cn, vec=None, groups=None):
    """(handle with groups, handle without) on the same vector"""
    vec = w.base if vec is None else vec
    gm = w.models[min_cn]
    a, b = gm.likelihood(w.rc, w.mp, vec, min_cn), gm.likelihood(w.rc, w.mp, vec, min_cn)
    goff, gnodes = w.groups if groups is None else groups
    a.set_groups(goff, gnodes)
    return a, b


def _bubble_swaps(w, n):
    """bubbles whose two arms are whole groups: hap-A-only arm +1, hap-B-only arm -1 with a floor of 0"""
    sg, (a, b) = w.sg, w.occ
    goff, gnodes = w.groups
    in_a, in_b = np.zeros(sg.base.size, bool), np.zeros(sg.base.size, bool)
    in_a[a] = True
    in_b[b] = True
    pos_b = {int(v): i for i, v in enumerate(b)}
    shared = np.flatnonzero(in_b[a])
    out = []
    for i in range(shared.size - 1):
        lo, hi = shared[i], shared[i + 1]
        if hi - lo < 3 or int(a[lo]) not in pos_b or int(a[hi]) not in pos_b:
            continue
        ib, jb = pos_b[int(a[lo])], pos_b[int(a[hi])]
        a_only = np.unique(a[lo + 1:hi][~in_b[a[lo + 1:hi]]])
        b_only = np.unique(b[ib + 1:jb][~in_a[b[ib + 1:jb]]]) if jb > ib else np.zeros(0, int)
        if a_only.size == 0 or b_only.size == 0:
            continue
        ga, gb = np.unique(w.group_of[a_only]), np.unique(w.group_of[b_only])
        whole = lambda gs, nodes: np.array_equal(  # noqa: E731
            np.sort(np.concatenate([gnodes[goff[g]:goff[g + 1]] for g in gs])), nodes)
        if not (whole(ga, a_only) and whole(gb, b_only)):
            continue
        gs = np.concatenate([ga, gb])
        vals = np.concatenate([w.gbase[ga].astype(np.int64) + 1, np.maximum(w.gbase[gb].astype(np.int64) - 1, 0)])
        out.append((gs, vals))
        if len(out) == n:
            break
    return out


def _random_group_cands(rng, gvec, n, ids=None):
    """n candidates of 1-4 random groups +-1 with a floor of 0"""
    ids = np.arange(gvec.size) if ids is None else ids
    out = []
    for _ in range(n):
        gs = rng.choice(ids, size=int(rng.integers(1, 5)), replace=False)
        out.append((gs, np.maximum(gvec[gs].astype(np.int64) + rng.choice([-1, 1], size=gs.size), 0)))
    return out


def _candidates(w, rng):
    sg, goff, gnodes = w.sg, *w.groups
    N = w.base.size
    cands = [([], [])]  # the empty list
    bubbles = _bubble_swaps(w, 10)
    assert len(bubbles) >= 6
    cands += bubbles
    cands += _random_group_cands(rng, w.gbase, 20)
    # the group holding the pad nodes together with emittable ones, +2
    pad = sg.base[gnodes] == D.graph.NULL_BASE
    n_pad = np.add.reduceat(pad.astype(np.int64), goff[:-1])
    g_pad = np.flatnonzero((n_pad > 0) & (n_pad < np.diff(goff)))
    assert g_pad.size >= 1
    cands.append(([g_pad[0]], [w.gbase[g_pad[0]] + 2]))
    # a group whose head is a child of a branching node: only a sibling's trans denominator changes
    outdeg = np.bincount(sg.edge_src, minlength=N)
    heads = gnodes[goff[:-1]]
    is_head = np.zeros(N, bool)
    is_head[heads] = True
    pick = [int(d) for s, d in zip(sg.edge_src, sg.edge_dst) if outdeg[s] >= 2 and is_head[d]]
    assert pick
    g_child = int(w.group_of[pick[0]])
    cands.append(([g_child], [w.gbase[g_child] + 1]))
    # every group to 0: at min_copy_num 0 this is T_c = 0, scored in full
    cands.append((np.arange(w.G), np.zeros(w.G, np.int64)))
    # one candidate naming 30 groups
    gs = rng.choice(w.G, size=30, replace=False)
    cands.append((gs, w.gbase[gs] + 1))
    return cands, len(bubbles)


def _assert_scores_equal(w, lk_g, lk_n, vec, gcands, min_cn, groups=None):
    """score_group_changes on lk_g == score_changes with the expanded lists on lk_n, and the rescored set is the
    node form's A_c restated in numpy -> (totals, per-read, n_rescored)"""
    groups = w.groups if groups is None else groups
    gch = _csr(gcands)
    nch = _csr(_expand(groups, gcands))
    tot_g, lp_g, n_g = lk_g.score_group_changes(gch)
    tot_n, lp_n, n_n = lk_n.score_changes(nch)
    exp = _expected_rescored(w.sg, vec, nch, min_cn, w.rc, w.mp.arrays())
    print("candidates", len(gcands), "group changes", gch[1].size, "node changes", nch[1].size,
          "rescored", n_g.tolist()[:8], "...")
    assert np.array_equal(n_g, n_n), (n_g, n_n)
    assert np.array_equal(n_g, exp.sum(axis=1)), (n_g, exp.sum(axis=1))
    assert np.array_equal(lp_g, lp_n)
    assert np.array_equal(tot_g, tot_n)
    tot_2, none, n_2 = lk_g.score_group_changes(gch, per_read=False)  # out_logp = NULL: no [C][R] matrix
    tot_3, none3, n_3 = lk_n.score_changes(nch, per_read=False)
    assert none is None and none3 is None
    assert np.array_equal(tot_2, tot_3) and np.array_equal(n_2, n_3)
    assert np.array_equal(tot_2, tot_g) and np.array_equal(n_2, n_g)
    return tot_g, lp_g, n_g


def _same_state(lk_g, lk_n):
    cg, vg, tg = lk_g.current()
    cn, vn, tn = lk_n.current()
    return np.array_equal(cg, cn) and np.array_equal(vg, vn) and tg == tn


@pytest.mark.parametrize("min_cn", [0, 1])
def test_score_equality(gpu_lib, world, min_cn):
    w = world
    lk_g, lk_n = _handles(w, min_cn)
    assert np.array_equal(lk_g.current_groups(), w.gbase)
    cands, n_bub = _candidates(w, np.random.default_rng(21))
    assert len(cands) >= 1 + 6 + 20 + 4
    tot, lp, nres = _assert_scores_equal(w, lk_g, lk_n, w.base, cands, min_cn)
    assert nres[0] == 0
    all_zero = 1 + n_bub + 20 + 2
    if min_cn == 0:
        assert nres[all_zero] == len(w.reads)  # T_c = 0: every non-empty read
    assert nres[1:1 + n_bub].min() > 0 and nres[-1] > 0
    assert _same_state(lk_g, lk_n)  # scoring moved nothing
    assert np.array_equal(lk_g.current_groups(), w.gbase)


@pytest.mark.parametrize("min_cn", [0, 1])
def test_chain_of_moves(gpu_lib, world, min_cn):
    w = world
    goff, gnodes = w.groups
    lk_g, lk_n = _handles(w, min_cn)
    rng = np.random.default_rng(40 + min_cn)
    gvec, vec = w.gbase.copy(), w.base.copy()
    moved = 0
    for it in range(30):
        cands = _random_group_cands(rng, gvec, 12)
        tot, lp, nres = _assert_scores_equal(w, lk_g, lk_n, vec, cands, min_cn)
        best = int(np.argmax(tot))
        gs, vals = cands[best]
        (nodes, nvals), = _expand(w.groups, [(gs, vals)])
        tg, ng = lk_g.move_groups(gs, vals)
        tn, nn = lk_n.move(nodes, nvals)
        assert tg == tn and ng == nn and ng == nres[best], (it, tg, tn, ng, nn)
        gvec[gs] = vals
        vec[nodes] = nvals
        moved += int(ng > 0)
        cg, vg, t_g = lk_g.current()
        cn, vn, t_n = lk_n.current()
        assert np.array_equal(cg, cn) and np.array_equal(cg, vec), it
        assert np.array_equal(vg, vn) and t_g == t_n, it
        cur_groups = lk_g.current_groups()
        assert np.array_equal(cur_groups, gvec), it
        through = np.empty_like(vec)
        through[gnodes] = np.repeat(cur_groups, np.diff(goff))
        assert np.array_equal(through, vec), it
    assert moved >= 15 and not np.array_equal(vec, w.base)
    tot_f, lp_f = w.models[min_cn].to_full_prob_reads_copy_nums(w.rc, w.mp, vec[None, :], min_cn)
    cur = lk_g.current()[1]
    print("after 30 moves: max |handle - full form| per read", float(np.nanmax(np.abs(cur - lp_f[0]))))
    assert _close(cur, lp_f[0], 1e-9)


def test_refusals(gpu_lib, world):
    w = world
    goff, gnodes = w.groups
    N, G = w.base.size, w.G
    lk_g, lk_n = _handles(w, 0)
    L = _ffi.lib()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    cands = _random_group_cands(np.random.default_rng(5), w.gbase, 5)
    off, grp, cn = _csr(cands)
    ref = lk_g.score_group_changes((off, grp, cn))
    state = lk_g.current()
    gstate = lk_g.current_groups()

    def unchanged():
        """the same scoring call gives the bits it gave before the refusal; vector, values, total and groups stand"""
        t, l, n = lk_g.score_group_changes((off, grp, cn))
        c, v, tt = lk_g.current()
        return (np.array_equal(t, ref[0]) and np.array_equal(l, ref[1]) and np.array_equal(n, ref[2])
                and np.array_equal(c, state[0]) and np.array_equal(v, state[1]) and tt == state[2]
                and np.array_equal(lk_g.current_groups(), gstate))

    out = np.full(5, 7.0)
    nout = np.full(5, 9, np.uint64)
    go64, gn32 = goff.astype(np.uint64), gnodes.astype(np.uint32)

    # set_groups: NULL arrays, group_off not starting at 0 / decreasing, a node id >= N, a node in two groups / twice
    bad_first = go64.copy()
    bad_first[0] = 1
    decreasing = go64.copy()
    decreasing[2] = decreasing[3] + 1
    big = gn32.copy()
    big[5] = N
    two = gn32.copy()
    two[int(go64[1])] = two[0]  # the first node of group 1 is the first node of group 0
    twice = gn32.copy()
    twice[1] = twice[0]
    assert go64[1] >= 2
    for o, nd in ((None, gn32), (go64, None), (bad_first, gn32), (decreasing, gn32), (go64, big), (go64, two),
                  (go64, twice)):
        assert L.phmm_likelihood_set_groups(lk_g._h, G, p(o), p(nd)) == _ffi.PHMM_EINVAL
        assert unchanged()
    # a vector that is not constant within a group
    split = np.array([0, 2], np.uint64)
    mixed_nodes = np.array([gnodes[goff[0]], gnodes[goff[1]]], np.uint32)
    other = np.flatnonzero(w.gbase != w.gbase[0])
    mixed_nodes[1] = gnodes[goff[other[0]]]
    assert L.phmm_likelihood_set_groups(lk_g._h, 1, p(split), p(mixed_nodes)) == _ffi.PHMM_EINVAL
    assert unchanged()

    # score_group_changes: NULL arrays, change_off, a group id >= G, a group named twice within one candidate
    c_bad_first = off.copy()
    c_bad_first[0] = 1
    c_decr = off.copy()
    c_decr[2] = c_decr[3] + 1
    c_big = grp.copy()
    c_big[0] = G
    two_off = np.array([0, 2], np.uint64)
    dup = np.array([grp[0], grp[0]], np.uint32)
    dup_cn = np.array([1, 1], np.uint32)
    for nc, o, g_, c_ in ((5, None, grp, cn), (5, off, None, cn), (5, off, grp, None), (5, c_bad_first, grp, cn),
                          (5, c_decr, grp, cn), (5, off, c_big, cn), (1, two_off, dup, dup_cn)):
        assert L.phmm_likelihood_score_group_changes(lk_g._h, nc, p(o), p(g_), p(c_), None, p(out),
                                                     p(nout)) == _ffi.PHMM_EINVAL
        assert np.all(out == 7.0) and np.all(nout == 9) and unchanged()
    # move_groups: the same
    for k, g_, c_ in ((2, None, dup_cn), (2, dup, None), (2, dup, dup_cn), (1, c_big[:1], cn[:1])):
        g_ = None if g_ is None else np.ascontiguousarray(g_)
        c_ = None if c_ is None else np.ascontiguousarray(c_)
        assert L.phmm_likelihood_move_groups(lk_g._h, k, p(g_), p(c_), p(out), p(nout)) == _ffi.PHMM_EINVAL
        assert np.all(out == 7.0) and np.all(nout == 9) and unchanged()
    gout = np.full(G, 5, np.uint32)
    assert L.phmm_likelihood_current_groups(lk_g._h, None) == _ffi.PHMM_EINVAL and unchanged()
    # n_candidates = 0 / n_changes = 0 as in the node form: success, nothing written, nothing changed
    assert L.phmm_likelihood_score_group_changes(lk_g._h, 0, p(off), p(grp), p(cn), None, p(out), p(nout)) == _ffi.PHMM_OK
    assert L.phmm_likelihood_move_groups(lk_g._h, 0, None, None, None, None) == _ffi.PHMM_OK
    assert np.all(out == 7.0) and np.all(nout == 9) and unchanged()

    # a group-form call with no groups set: on the handle that never had any, and after n_groups = 0
    for lk in (lk_n, None):
        if lk is None:
            lk_g.set_groups(np.zeros(0, np.uint64), np.zeros(0, np.uint32))
            lk = lk_g
        assert L.phmm_likelihood_score_group_changes(lk._h, 5, p(off), p(grp), p(cn), None, p(out),
                                                     p(nout)) == _ffi.PHMM_EINVAL
        assert L.phmm_likelihood_move_groups(lk._h, 1, p(grp), p(cn), p(out), p(nout)) == _ffi.PHMM_EINVAL
        assert L.phmm_likelihood_current_groups(lk._h, p(gout)) == _ffi.PHMM_EINVAL
        assert np.all(out == 7.0) and np.all(nout == 9) and np.all(gout == 5)
        assert b"no groups" in L.phmm_last_error()
    assert _same_state(lk_g, lk_n)
    lk_g.set_groups(goff, gnodes)  # ... and back: the same bits as before all of it
    assert unchanged()
    # the node form on the handle with groups is what it is on the handle without
    nch = _csr(_expand(w.groups, cands))
    t_a, l_a, n_a = lk_g.score_changes(nch)
    t_b, l_b, n_b = lk_n.score_changes(nch)
    assert np.array_equal(t_a, t_b) and np.array_equal(l_a, l_b) and np.array_equal(n_a, n_b)
    assert np.array_equal(t_a, ref[0]) and np.array_equal(l_a, ref[1]) and np.array_equal(n_a, ref[2])


def test_mixed_groups(gpu_lib, world):
    w = world
    goff, gnodes = w.groups
    lk_g, lk_n = _handles(w, 0)
    sizes = np.diff(goff)
    g = int(np.flatnonzero((sizes >= 10) & (sizes <= 40))[3])
    half = gnodes[goff[g]:goff[g] + sizes[g] // 2]
    rest = gnodes[goff[g] + sizes[g] // 2:goff[g + 1]]
    new = np.full(half.size, w.gbase[g] + 1, np.uint32)
    ta, na = lk_g.move(half, new)  # a node-form move that changes half of one group
    tb, nb = lk_n.move(half, new)
    assert ta == tb and na == nb and _same_state(lk_g, lk_n)
    vec = w.base.copy()
    vec[half] = new
    cur = lk_g.current_groups()
    want = w.gbase.copy()
    want[g] = MIXED
    assert np.array_equal(cur, want)
    # a group-form candidate naming it is refused (nothing written); one that does not is scored and equals the node form
    L = _ffi.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    others = np.array([x for x in range(w.G) if x != g])
    rng = np.random.default_rng(9)
    good = _random_group_cands(rng, w.gbase, 6, ids=others)
    ref = _assert_scores_equal(w, lk_g, lk_n, vec, good, 0)
    off, grp, cn = _csr(good + [([g], [w.gbase[g] + 1])])
    out, nout = np.full(7, 7.0), np.full(7, 9, np.uint64)
    assert L.phmm_likelihood_score_group_changes(lk_g._h, 7, p(off), p(grp), p(cn), None, p(out),
                                                 p(nout)) == _ffi.PHMM_EINVAL
    assert b"mixed" in L.phmm_last_error()
    one_g, one_c = np.array([g], np.uint32), np.array([1], np.uint32)
    assert L.phmm_likelihood_move_groups(lk_g._h, 1, p(one_g), p(one_c), p(out), p(nout)) == _ffi.PHMM_EINVAL
    assert np.all(out == 7.0) and np.all(nout == 9) and _same_state(lk_g, lk_n)
    again = _assert_scores_equal(w, lk_g, lk_n, vec, good, 0)
    assert all(np.array_equal(a, b) for a, b in zip(ref, again))
    # set_groups with the same groups is now refused; the groups in force stay as they were
    assert L.phmm_likelihood_set_groups(lk_g._h, w.G, p(goff.astype(np.uint64)), p(gnodes)) == _ffi.PHMM_EINVAL
    assert np.array_equal(lk_g.current_groups(), want)
    # with that group split in two it is accepted, and the halves can be changed
    cut = goff[g] + sizes[g] // 2
    goff2 = np.concatenate([goff[:g + 1], [cut], goff[g + 1:]])
    lk_g.set_groups(goff2, gnodes)
    want2 = np.concatenate([w.gbase[:g], [w.gbase[g] + 1, w.gbase[g]], w.gbase[g + 1:]])
    assert np.array_equal(lk_g.current_groups(), want2)
    halves = [([g], [want2[g] + 1]), ([g + 1], [want2[g + 1] + 2]), ([g, g + 1], [0, 3])]
    _assert_scores_equal(w, lk_g, lk_n, vec, halves, 0, groups=(goff2, gnodes))
    tg, ng = lk_g.move_groups([g, g + 1], [0, 3])
    vec[half], vec[rest] = 0, 3
    tn, nn = lk_n.move(np.concatenate([half, rest]), vec[np.concatenate([half, rest])])
    assert tg == tn and ng == nn and _same_state(lk_g, lk_n) and np.array_equal(lk_g.current()[0], vec)
    # a node-form move that gives every node of a group one value leaves it uniform at that value
    whole = gnodes[goff2[g]:goff2[g + 1]]
    lk_g.move(whole, np.full(whole.size, 2, np.uint32))
    assert lk_g.current_groups()[g] == 2
    lk_g.refresh()  # refresh does not touch the groups
    assert lk_g.current_groups()[g] == 2 and lk_g.current_groups()[g + 1] == 3


def test_partial_cover(gpu_lib, world):
    """groups over every second unitig only; the other nodes are in no group (boundary parents among them)"""
    w = world
    goff, gnodes = w.groups
    keep = np.arange(0, w.G, 2)
    nodes2 = np.concatenate([gnodes[goff[g]:goff[g + 1]] for g in keep])
    off2 = np.concatenate([[0], np.cumsum(np.diff(goff)[keep])])
    gbase2 = w.gbase[keep]
    for min_cn in (0, 1):
        lk_g, lk_n = _handles(w, min_cn, groups=(off2, nodes2))
        assert np.array_equal(lk_g.current_groups(), gbase2)
        rng = np.random.default_rng(17)
        cands = [([], [])] + _random_group_cands(rng, gbase2, 20)
        cands.append((np.arange(keep.size), np.zeros(keep.size, np.int64)))
        gs = rng.choice(keep.size, size=30, replace=False)
        cands.append((gs, gbase2[gs] + 1))
        tot, lp, nres = _assert_scores_equal(w, lk_g, lk_n, w.base, cands, min_cn, groups=(off2, nodes2))
        assert nres[0] == 0 and nres[-1] > 0
        gs, vals = cands[-1]
        (nodes, nvals), = _expand((off2, nodes2), [(gs, vals)])
        assert lk_g.move_groups(gs, vals) == lk_n.move(nodes, nvals) and _same_state(lk_g, lk_n)


def test_steady_state(gpu_lib, world):
    """phmm_workspace_bytes() is the same after the second and the fourth identical score_group_changes."""
    w = world
    lk_g, lk_n = _handles(w, 0)
    cands, _ = _candidates(w, np.random.default_rng(21))
    gch = _csr(cands)
    ws, outs = [], []
    for _ in range(4):
        outs.append(lk_g.score_group_changes(gch))
        ws.append(gpu_lib.phmm_workspace_bytes())
    assert ws[1] == ws[3], ws
    for o in outs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(o, outs[0]))
    # ... also through moves there and back
    gs, vals = cands[1]
    for _ in range(2):
        lk_g.move_groups(gs, vals)
        lk_g.move_groups(gs, w.gbase[gs])
        lk_g.score_group_changes(gch, per_read=False)
        ws.append(gpu_lib.phmm_workspace_bytes())
    assert ws[-1] == ws[-2], ws
    assert np.array_equal(lk_g.current()[0], w.base)
