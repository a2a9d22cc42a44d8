"""GPU: the sampler's state on the device (phmm_likelihood), the greedy search of sample_posterior
(multi_dbg/posterior.rs:314-417): score_changes against the handle's current vector equals the stateless change form
called with that vector as its base, and a move leaves what the full form (phmm_full_prob_reads_copy_nums) computes on
the new vector -- rescored reads bit-equal, every other read within 1e-9, totals within 1e-9 * R -- also after a chain
of 30 moves.  The small diploid, the bubble swaps and the numpy restatement of the rescored set are those of
test_gpu_copy_num_changes.py (restated: a test module cannot be imported without editing it)."""
import ctypes as C

import numpy as np
import pytest

import dbgphmm_amd as D
from dbgphmm_amd import _ffi
from helpers import subset_csr
import repeat_cases

pytestmark = pytest.mark.gpu
K = 20


def _close(a, b, tol):
    a, b = np.asarray(a, float), np.asarray(b, float)
    both_inf = np.isneginf(a) & np.isneginf(b)
    with np.errstate(invalid="ignore"):
        return bool(np.all(both_inf | (np.abs(a - b) <= tol)))


def _materialise(base, changes):
    off, node, cn = changes
    out = np.repeat(base[None, :], off.size - 1, axis=0)
    for c in range(off.size - 1):
        out[c, node[off[c]:off[c + 1]]] = cn[off[c]:off[c + 1]]
    return out


def _csr(base, cand_changes):
    """[(nodes, new cns)] per candidate -> (off, node, cn)"""
    off = np.zeros(len(cand_changes) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(n) for n, _ in cand_changes])
    node = np.concatenate([np.asarray(n, np.uint32) for n, _ in cand_changes] + [np.zeros(0, np.uint32)])
    cn = np.concatenate([np.asarray(v, np.uint32) for _, v in cand_changes] + [np.zeros(0, np.uint32)])
    return off, node, cn


def _expected_rescored(sg, base, changes, min_cn, rc, mp_arrays):
    """per candidate: non-empty reads whose lists meet A_c = D_c + parents(D_c); all non-empty reads when T_c or
    T_base is 0"""
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


@pytest.fixture(scope="module")
def diploid():
    hap = D.random_genome(12000, seed=11)
    haps = [hap, D.diverge(hap, 0.01, seed=12)]
    sg, occ = D.dbg_from_haplotypes(haps, K, with_occurrences=True)
    param = D.PHMMParams.uniform(0.001).with_(n_warmup=K)
    a1 = D.vectorised_to_phmm(sg, param, 1)
    reads = D.sample_reads(a1, 10 ** 9, 1000, seed=13, max_reads=240)
    rc = D.ReadCollection(reads)
    mp, _ = D.PHMMModel(a1).generate_mappings(rc, None, True)
    return sg, occ, param, reads, rc, mp


def _bubble_swaps(sg, occ, n):
    """between two k-mers both haplotypes share: hap-A-only k-mers +1, hap-B-only k-mers -1"""
    a, b = occ
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
        nodes = np.concatenate([a_only, b_only])
        vals = np.concatenate([sg.copy_num[a_only] + 1, np.maximum(sg.copy_num[b_only] - 1, 0)])
        out.append((nodes, vals))
        if len(out) == n:
            break
    return out


def _candidates(sg, occ, rng):
    """the candidate set of test_change_form_matches_full_form"""
    base = sg.copy_num.astype(np.uint32)
    N = base.size
    cands = [([], [])]  # empty change list
    for _ in range(20):  # bench's shape: random k-mers +-1
        ix = np.unique(rng.integers(0, N, size=16))
        cands.append((ix, np.maximum(base[ix].astype(np.int64) + rng.choice([-1, 1], size=ix.size), 0)))
    bubbles = _bubble_swaps(sg, occ, 10)
    assert len(bubbles) >= 6
    cands += bubbles
    # a change that only alters a sibling's trans denominator: a child of a branching node
    outdeg = np.bincount(sg.edge_src, minlength=N)
    u = int(np.flatnonzero(outdeg >= 2)[0])
    w = int(sg.edge_dst[np.flatnonzero(sg.edge_src == u)[0]])
    cands.append(([w], [base[w] + 1]))
    # changes on n pad nodes
    pads = np.flatnonzero(sg.base == D.graph.NULL_BASE)[:4]
    cands.append((pads, base[pads] + 2))
    # every emittable node to 0: T_c = 0, scored in full
    cands.append((np.arange(N), np.zeros(N, np.int64)))
    # a larger move across a few unitigs
    ix = rng.integers(0, N, size=200)
    ix = np.unique(ix)
    cands.append((ix, base[ix] + 1))
    return base, _csr(base, cands), len(bubbles)


def _check_scoring(gm, lk, sg, rc, mp, base, changes, min_cn):
    """score_changes through the handle (current vector = base) against the stateless change form on `base`"""
    R = len(rc)
    tot_s, lp_s, n_s = gm.to_full_prob_reads_copy_num_changes(rc, mp, base, changes, min_cn)
    tot, lp, nres = lk.score_changes(changes)
    exp = _expected_rescored(sg, base, changes, min_cn, rc, mp.arrays())
    assert np.array_equal(nres, n_s) and np.array_equal(nres, exp.sum(axis=1)), (nres, n_s, exp.sum(axis=1))
    for c in range(exp.shape[0]):
        assert np.array_equal(lp[c][exp[c]], lp_s[c][exp[c]]), c  # rescored pairs: the same bits
        assert _close(lp[c], lp_s[c], 1e-9), c
    assert _close(tot, tot_s, 1e-9 * R)
    # the same bits on a second call; totals alone (no [C][R] matrix) are the same totals
    tot2, lp2, nres2 = lk.score_changes(changes)
    assert np.array_equal(lp2, lp) and np.array_equal(tot2, tot) and np.array_equal(nres2, nres)
    tot3, none, nres3 = lk.score_changes(changes, per_read=False)
    assert none is None and np.array_equal(tot3, tot) and np.array_equal(nres3, nres)
    return tot, lp, nres, exp


def _check_move(gm, lk, sg, rc, mp, vec, nodes, vals, min_cn):
    """one move against the full form on the new vector -> (new vector, rescored mask)"""
    R = len(rc)
    one = _csr(vec, [(nodes, vals)])
    exp = _expected_rescored(sg, vec, one, min_cn, rc, mp.arrays())[0]
    tot, n = lk.move(nodes, vals)
    new = _materialise(vec, one)[0]
    cur_cn, cur_lp, cur_tot = lk.current()
    assert np.array_equal(cur_cn, new)
    assert n == int(exp.sum()), (n, int(exp.sum()))
    tot_f, lp_f = gm.to_full_prob_reads_copy_nums(rc, mp, new[None, :], min_cn)
    assert np.array_equal(cur_lp[exp], lp_f[0][exp])  # rescored reads: the same bits
    assert np.all(np.isfinite(cur_lp) == np.isfinite(lp_f[0]))
    assert _close(cur_lp, lp_f[0], 1e-9)
    assert _close(tot, tot_f[0], 1e-9 * R) and tot == cur_tot
    return new, exp


def test_score_changes_equals_stateless_form(gpu_lib, diploid):
    sg, occ, param, reads, rc, mp = diploid
    rng = np.random.default_rng(21)
    base, changes, n_bub = _candidates(sg, occ, rng)
    gm = D.PHMMModel(D.vectorised_to_phmm(sg, param, 0))
    lk = gm.likelihood(rc, mp, base, 0)
    assert 35 <= changes[0].size - 1 <= 45
    tot, lp, nres, exp = _check_scoring(gm, lk, sg, rc, mp, base, changes, 0)
    assert nres[0] == 0 and nres[-2] == len(reads)  # empty list: nothing; T_c = 0: every non-empty read
    # what the handle holds is the full form on the base; the empty candidate is that
    tot_f, lp_f = gm.to_full_prob_reads_copy_nums(rc, mp, base[None, :], 0)
    cn, cur, cur_tot = lk.current()
    assert np.array_equal(cn, base) and np.array_equal(cur, lp_f[0]) and np.array_equal(lp[0], cur)
    assert _close(cur_tot, tot_f[0], 1e-9 * len(reads))


def test_min_copy_num_one(gpu_lib, diploid):
    sg, occ, param, reads, rc, mp = diploid
    base = sg.copy_num.astype(np.uint32)
    gm = D.PHMMModel(D.vectorised_to_phmm(sg, param, 1))
    lk = gm.likelihood(rc, mp, base, 1)
    ones = np.flatnonzero(base == 1)[:3]
    rng = np.random.default_rng(3)
    ix = np.unique(rng.integers(0, base.size, size=16))
    changes = _csr(base, [(ones, [0, 0, 0]), (ix, base[ix] + 1), ([], [])])
    tot, lp, nres, exp = _check_scoring(gm, lk, sg, rc, mp, base, changes, 1)
    assert nres[0] == 0 and nres[2] == 0  # 1 -> 0 under min_copy_num 1 changes nothing
    assert np.array_equal(lp[0], lp[2])
    # ... and as a move it rescored nothing, yet the vector holds the zeros
    vec, hit = _check_move(gm, lk, sg, rc, mp, base, ones, [0, 0, 0], 1)
    assert not hit.any() and np.all(vec[ones] == 0)
    _check_move(gm, lk, sg, rc, mp, vec, ix, base[ix] + 1, 1)


def _oracle_check(oracle, sg, param, reads, rc, mp, vec, cur_lp, base_lp, touched):
    off = rc.offsets.astype(np.int64)
    hit, clean = np.flatnonzero(touched), np.flatnonzero(~touched & (np.diff(off) > 0))
    assert hit.size >= 6 and clean.size >= 6
    sample = np.unique(np.concatenate([hit[:6], clean[:6]]))
    sub = [reads[r] for r in sample]
    with np.errstate(divide="ignore"):
        ac = D.vectorised_to_phmm(D.SeqGraph(vec.astype(np.int64), sg.base, sg.edge_src, sg.edge_dst, None), param, 0)
    ol = oracle.Model(ac).full_prob_reads(sub, subset_csr(off, mp.arrays(), sample), True, n_threads=8)
    cut = base_lp[sample] - ol > 100.0
    tol = np.where(cut, 1e-6, 1e-9)
    with np.errstate(invalid="ignore"):
        assert np.all((np.isneginf(ol) & np.isneginf(cur_lp[sample])) | (np.abs(ol - cur_lp[sample]) <= tol))


def test_chain_of_moves_is_the_full_form(gpu_lib, oracle, diploid):
    sg, occ, param, reads, rc, mp = diploid
    base = sg.copy_num.astype(np.uint32)
    R = len(reads)
    gm = D.PHMMModel(D.vectorised_to_phmm(sg, param, 0))
    lk = gm.likelihood(rc, mp, base, 0)
    base_lp = lk.current()[1]
    bubbles, used = [], np.zeros(base.size, bool)
    for nodes, vals in _bubble_swaps(sg, occ, 40):  # node-disjoint ones
        if not used[nodes].any():
            used[nodes] = True
            bubbles.append((nodes.astype(np.uint32), vals.astype(np.uint32)))
    assert len(bubbles) >= 26
    cuts = [i for i, (n, v) in enumerate(bubbles[:12]) if np.any(v == 0)]
    assert cuts, "no swap sets a hap-B-only k-mer to 0"
    restore = lambda i: (bubbles[i][0], base[bubbles[i][0]])  # noqa: E731
    moves = [bubbles[i] for i in range(12)]
    moves.append((np.zeros(0, np.uint32), np.zeros(0, np.uint32)))  # n_changes = 0
    moves.append((np.concatenate([bubbles[i][0] for i in (12, 13, 14)]),
                  np.concatenate([bubbles[i][1] for i in (12, 13, 14)])))  # a multi-move: the union of three
    moves += [restore(i) for i in (cuts + [i for i in range(12) if i not in cuts])[:6]]
    moves += [bubbles[i] for i in range(15, 25)]
    assert len(moves) == 30
    vec, touched, any_cut = base.copy(), np.zeros(R, bool), False
    for i, (nodes, vals) in enumerate(moves):
        vec, hit = _check_move(gm, lk, sg, rc, mp, vec, nodes, vals, 0)
        touched |= hit
        if nodes.size == 0:
            assert not hit.any()
        cur = lk.current()[1]
        # (a hap-B read over a zeroed hap-B-only k-mer pays at least one mismatch, ln 0.001, to get past it)
        any_cut |= bool(np.any(base_lp[hit] - cur[hit] > 1.0))
        if i == 9 or i == len(moves) - 1:
            _oracle_check(oracle, sg, param, reads, rc, mp, vec, cur, base_lp, touched)
    assert any_cut, "no move cut a read"
    assert (~touched & (np.diff(rc.offsets.astype(np.int64)) > 0)).sum() >= 6
    # from the final vector: ten fresh candidates as the stateless form scores them with that vector as its base
    rng = np.random.default_rng(33)
    chs = []
    for _ in range(8):
        ix = np.unique(rng.integers(0, base.size, size=16))
        chs.append((ix, np.maximum(vec[ix].astype(np.int64) + rng.choice([-1, 1], size=ix.size), 0)))
    chs += [(bubbles[25][0], bubbles[25][1]), restore(11)]
    _check_scoring(gm, lk, sg, rc, mp, vec, _csr(vec, chs), 0)
    before = lk.current()[1]
    lk.refresh()
    cn, after, _ = lk.current()
    assert np.array_equal(cn, vec) and _close(after, before, 1e-9)
    assert np.array_equal(after, gm.to_full_prob_reads_copy_nums(rc, mp, vec[None, :], 0)[1][0])


class _DeviceArray:
    """n 8-byte elements in device memory (the HIP runtime the library is linked against)"""

    def __init__(self, n):
        self.hip, self.n = C.CDLL("libamdhip64.so"), n
        self.p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.p), C.c_size_t(8 * max(n, 1))) == 0

    def numpy(self, dtype=np.float64):
        out = np.empty(self.n, dtype=dtype)
        assert self.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), self.p, C.c_size_t(8 * self.n), 2) == 0
        return out

    def __del__(self):
        self.hip.hipFree(self.p)


def test_state_and_refusals(gpu_lib, diploid):
    """Refusals are the argument checks of the contract.  A move that fails half-way (capacity, out of memory) is not
    provoked here -- there is no honest way to make the device run out on demand; the code commits the state only
    behind its last fallible step (sparse.hip, likelihood_move)."""
    sg, occ, param, reads, rc, mp = diploid
    base = sg.copy_num.astype(np.uint32)
    R = len(reads)
    gm = D.PHMMModel(D.vectorised_to_phmm(sg, param, 0))
    lk = gm.likelihood(rc, mp, base, 0)
    rng = np.random.default_rng(8)
    chs = []
    for _ in range(5):
        ix = np.unique(rng.integers(0, base.size, size=16))
        chs.append((ix, base[ix] + 1))
    off, node, cn = _csr(base, chs)
    tot, lp, nres = lk.score_changes((off, node, cn))
    L = _ffi.lib()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def state():
        c, v, t = lk.current()
        return c, v, t

    def same_state(s):
        c, v, t = lk.current()
        return np.array_equal(c, s[0]) and np.array_equal(v, s[1]) and t == s[2]

    # device-pointer outputs equal host outputs
    dlp, dtot, dn = _DeviceArray(5 * R), _DeviceArray(5), _DeviceArray(5)
    assert L.phmm_likelihood_score_changes(lk._h, 5, p(off), p(node), p(cn), dlp.p, dtot.p, dn.p) == _ffi.PHMM_OK
    assert np.array_equal(dlp.numpy().reshape(5, -1), lp) and np.array_equal(dtot.numpy(), tot)
    assert np.array_equal(dn.numpy(np.uint64), nres)
    dcur, dct = _DeviceArray(R), _DeviceArray(1)
    s0 = state()
    assert L.phmm_likelihood_current(lk._h, None, dcur.p, dct.p) == _ffi.PHMM_OK
    assert np.array_equal(dcur.numpy(), s0[1]) and dct.numpy()[0] == s0[2]
    # ... also those of a move (and of the move back)
    mt, mn = _DeviceArray(1), _DeviceArray(1)
    n0_, v0_ = np.ascontiguousarray(chs[0][0], np.uint32), np.ascontiguousarray(chs[0][1], np.uint32)
    back_ = np.ascontiguousarray(base[n0_])
    assert L.phmm_likelihood_move(lk._h, n0_.size, p(n0_), p(v0_), mt.p, mn.p) == _ffi.PHMM_OK
    assert mt.numpy()[0] == lk.current()[2] and mn.numpy(np.uint64)[0] == nres[0]
    ht, hn = lk.move(n0_, back_)
    assert hn == nres[0] and same_state(s0)
    # NULL outputs are fine; n_candidates = 0 / n_changes = 0 succeed and change nothing
    assert L.phmm_likelihood_score_changes(lk._h, 5, p(off), p(node), p(cn), None, None, None) == _ffi.PHMM_OK
    sentinel = np.full(3, 7.0)
    assert L.phmm_likelihood_score_changes(lk._h, 0, p(off), p(node), p(cn), None, p(sentinel), None) == _ffi.PHMM_OK
    assert np.all(sentinel == 7.0)
    assert L.phmm_likelihood_move(lk._h, 0, None, None, None, None) == _ffi.PHMM_OK
    assert same_state(s0)
    # refusals: PHMM_EINVAL, nothing written, the state as before
    out = np.full(5, 7.0)
    nout = np.full(5, 9, np.uint64)
    bad_first = off.copy()
    bad_first[0] = 1
    decreasing = off.copy()
    decreasing[2] = decreasing[3] + 1
    big = node.copy()
    big[3] = base.size
    dup = node.copy()
    dup[1] = dup[0]
    for o, nd, c in ((bad_first, node, cn), (decreasing, node, cn), (off, big, cn), (off, dup, cn), (None, node, cn),
                     (off, None, cn), (off, node, None)):
        assert L.phmm_likelihood_score_changes(lk._h, 5, p(o), p(nd), p(c), None, p(out), p(nout)) == _ffi.PHMM_EINVAL
        assert np.all(out == 7.0) and np.all(nout == 9) and same_state(s0)
    assert L.phmm_likelihood_score_changes(None, 5, p(off), p(node), p(cn), None, p(out), None) == _ffi.PHMM_EINVAL
    n0 = int(off[1])
    for nd, c in ((big[:n0 + 4], cn[:n0 + 4]), (dup[:n0], cn[:n0]), (None, cn[:n0]), (node[:n0], None)):
        k = n0 if nd is None or c is None else nd.size
        nd = None if nd is None else np.ascontiguousarray(nd)
        c = None if c is None else np.ascontiguousarray(c)
        assert L.phmm_likelihood_move(lk._h, k, p(nd), p(c), p(out), p(nout)) == _ffi.PHMM_EINVAL
        assert np.all(out == 7.0) and np.all(nout == 9) and same_state(s0)
    assert L.phmm_likelihood_move(None, n0, p(node), p(cn), p(out), None) == _ffi.PHMM_EINVAL and np.all(out == 7.0)
    # create: NULL copy numbers / mappings, mappings of another read set, node degree above 8
    other = D.ReadCollection(reads[:10])
    other_mp, _ = gm.generate_mappings(other, None, True)
    for mph, b in ((mp._h, None), (None, base), (other_mp._h, base)):
        h = C.c_void_p(0x1234)
        assert L.phmm_likelihood_create(gm._h, rc._h, mph, p(b), 0, C.byref(h)) == _ffi.PHMM_EINVAL and not h.value
    assert L.phmm_likelihood_create(gm._h, rc._h, mp._h, p(base), 0, None) == _ffi.PHMM_EINVAL
    n = 12
    hub = D.SeqGraph(np.ones(n, dtype=np.int64), np.frombuffer(b"ACGTACGTACGT", dtype=np.uint8).copy(),
                     np.array(list(range(1, 11)), dtype=np.uint32), np.array([0] * 10, dtype=np.uint32), None)
    hm = D.PHMMModel(D.vectorised_to_phmm(hub, D.PHMMParams.uniform(0.01).with_(n_warmup=2), 1))
    hr = D.ReadCollection([b"ACG"])
    hmp = D.Mappings.from_arrays(hr, np.arange(4, dtype=np.uint64), np.zeros(3, np.uint32), np.zeros(3))
    h = C.c_void_p(0x1234)
    assert L.phmm_likelihood_create(hm._h, hr._h, hmp._h, p(np.ones(n, np.uint32)), 0,
                                    C.byref(h)) == _ffi.PHMM_EINVAL and not h.value
    assert same_state(s0)

    # the handle's arrays are its own: releasing the workspace between two calls changes no bit
    assert gpu_lib.phmm_release_workspace() == _ffi.PHMM_OK
    tot2, lp2, nres2 = lk.score_changes((off, node, cn))
    assert np.array_equal(lp2, lp) and np.array_equal(tot2, tot) and np.array_equal(nres2, nres) and same_state(s0)

    # steady state: no workspace growth between the second and the fourth identical round
    nodes0, vals0 = chs[0]
    ws, rounds = [], []
    for _ in range(4):
        t, l, n_ = lk.score_changes((off, node, cn))
        m1 = lk.move(nodes0, vals0)
        m2 = lk.move(nodes0, base[nodes0])
        rounds.append((t, l, n_, m1, m2))
        ws.append(gpu_lib.phmm_workspace_bytes())
        assert np.array_equal(lk.current()[0], base)
    assert ws[1] == ws[3]
    for r in rounds[1:]:  # the same state, the same bits
        assert np.array_equal(r[0], rounds[0][0]) and np.array_equal(r[2], rounds[0][2]) and r[3:] == rounds[0][3:]
        assert np.array_equal(r[1], rounds[0][1])

    # two handles on one model / read set / mappings do not disturb each other
    other_vec = base.copy()
    other_vec[chs[1][0]] = chs[1][1]
    lk2 = gm.likelihood(rc, mp, other_vec, 0)
    s1, s2 = state(), lk2.current()
    lk2.move(chs[2][0], chs[2][1])
    assert same_state(s1)
    lk.move(chs[3][0], chs[3][1])
    moved = other_vec.copy()
    moved[chs[2][0]] = chs[2][1]
    c2, v2, _ = lk2.current()
    assert np.array_equal(c2, moved)
    _check_scoring(gm, lk2, sg, rc, mp, moved, _csr(moved, chs[3:]), 0)
    assert _close(v2, gm.to_full_prob_reads_copy_nums(rc, mp, moved[None, :], 0)[1][0], 1e-9)
    assert not np.array_equal(s2[0], c2)


def test_wide_lists(gpu_lib):
    """tandem repeat: lists past 32, 64 and 128 nodes, so that pairs run in the one-candidate and 400-slot classes"""
    arrays, reads, sg, haps = repeat_cases.dataset("u100", 40, max_reads=60)
    gm1 = D.PHMMModel(arrays)
    rc = D.ReadCollection(reads)
    mp, _ = gm1.generate_mappings(rc, None, True)
    po = mp.arrays()[0].astype(np.int64)
    off = rc.offsets.astype(np.int64)
    cnt = np.diff(po)
    read_max = np.array([cnt[off[r]:off[r + 1]].max() if off[r + 1] > off[r] else 0 for r in range(len(reads))])
    base = sg.copy_num.astype(np.uint32)
    rng = np.random.default_rng(5)
    chs = [([], [])]
    for _ in range(7):
        ix = np.unique(rng.integers(0, base.size, size=16))
        chs.append((ix, np.maximum(base[ix].astype(np.int64) + rng.choice([-1, 1], size=ix.size), 1)))
    changes = _csr(base, chs)
    gm = D.PHMMModel(D.vectorised_to_phmm(sg, arrays.param, 0))
    lk = gm.likelihood(rc, mp, base, 0)
    tot, lp, nres, exp = _check_scoring(gm, lk, sg, rc, mp, base, changes, 0)
    assert (exp & (read_max[None, :] > 128)).any()
    long_hits = (exp & (read_max[None, :] > 128)).sum(axis=1)
    vec, hit_long = base, False
    for c in np.argsort(-long_hits, kind="stable")[:3]:  # (the first one moves from the base: its reads are exp[c])
        nodes, vals = chs[c]
        vec, hit = _check_move(gm, lk, sg, rc, mp, vec, np.asarray(nodes, np.uint32), np.asarray(vals, np.uint32), 0)
        hit_long |= bool((hit & (read_max > 128)).any())
    assert hit_long
