"""GPU: candidates given as changes to a base copy-number vector (phmm_full_prob_reads_copy_num_changes), the loop of
sample_posterior_once (multi_dbg/posterior.rs:483-515) rescoring only the reads a candidate touches.  The yardstick is
the full form (phmm_full_prob_reads_copy_nums) on the materialised vectors: rescored pairs bit-equal, every read within
1e-9; the set of rescored reads is restated here in numpy."""
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


def test_change_form_matches_full_form(gpu_lib, oracle, diploid):
    sg, occ, param, reads, rc, mp = diploid
    rng = np.random.default_rng(21)
    base, changes, n_bub = _candidates(sg, occ, rng)
    a0 = D.vectorised_to_phmm(sg, param, 0)
    gm = D.PHMMModel(a0)
    cands = _materialise(base, changes)
    Cn = cands.shape[0]
    assert 35 <= Cn <= 45
    tot_f, lp_f = gm.to_full_prob_reads_copy_nums(rc, mp, cands, 0)
    tot, lp, nres = gm.to_full_prob_reads_copy_num_changes(rc, mp, base, changes, 0)
    R = len(reads)
    exp = _expected_rescored(sg, base, changes, 0, rc, mp.arrays())
    assert np.array_equal(nres, exp.sum(axis=1)), (nres, exp.sum(axis=1))
    assert nres[0] == 0 and nres[-2] == R  # empty list: nothing; T_c = 0: every non-empty read
    for c in range(Cn):
        assert np.array_equal(lp[c][exp[c]], lp_f[c][exp[c]]), c  # rescored pairs: the same bits
        assert _close(lp[c], lp_f[c], 1e-9), c
    assert _close(tot, tot_f, 1e-9 * R)
    # a candidate alone gives the bits it has in the batch; two calls give the same bits; no workspace growth
    for c in (3, 22, Cn - 1):
        one = _csr(base, [(changes[1][changes[0][c]:changes[0][c + 1]], changes[2][changes[0][c]:changes[0][c + 1]])])
        t1, l1, n1 = gm.to_full_prob_reads_copy_num_changes(rc, mp, base, one, 0)
        assert np.array_equal(l1[0], lp[c]) and n1[0] == nres[c] and t1[0] == tot[c]
    ws = gpu_lib.phmm_workspace_bytes()
    tot2, lp2, nres2 = gm.to_full_prob_reads_copy_num_changes(rc, mp, base, changes, 0)
    assert np.array_equal(lp2, lp) and np.array_equal(tot2, tot) and np.array_equal(nres2, nres)
    assert gpu_lib.phmm_workspace_bytes() == ws
    # the oracle on the host-built model of three candidates, on a sample of clean and rescored reads
    off = rc.offsets.astype(np.int64)
    mpa = mp.arrays()
    for c in (5, 21, 21 + n_bub):
        hit, clean = np.flatnonzero(exp[c]), np.flatnonzero(~exp[c] & (np.diff(off) > 0))
        sample = np.unique(np.concatenate([hit[:6], clean[:6]]))
        sub = [reads[r] for r in sample]
        with np.errstate(divide="ignore"):
            ac = D.vectorised_to_phmm(D.SeqGraph(cands[c].astype(np.int64), sg.base, sg.edge_src, sg.edge_dst, None),
                                      param, 0)
        ol = oracle.Model(ac).full_prob_reads(sub, subset_csr(off, mpa, sample), True, n_threads=8)
        cut = lp[0][sample] - ol > 100.0
        tol = np.where(cut, 1e-6, 1e-9)
        with np.errstate(invalid="ignore"):
            assert np.all((np.isneginf(ol) & np.isneginf(lp[c][sample])) | (np.abs(ol - lp[c][sample]) <= tol)), c


def test_min_copy_num_one_and_no_effect(gpu_lib, diploid):
    sg, occ, param, reads, rc, mp = diploid
    base = sg.copy_num.astype(np.uint32)
    gm = D.PHMMModel(D.vectorised_to_phmm(sg, param, 1))
    ones = np.flatnonzero(base == 1)[:3]
    rng = np.random.default_rng(3)
    ix = np.unique(rng.integers(0, base.size, size=16))
    changes = _csr(base, [(ones, [0, 0, 0]), (ix, base[ix] + 1), ([], [])])
    tot, lp, nres = gm.to_full_prob_reads_copy_num_changes(rc, mp, base, changes, 1)
    tot_f, lp_f = gm.to_full_prob_reads_copy_nums(rc, mp, _materialise(base, changes), 1)
    assert nres[0] == 0 and nres[2] == 0  # 1 -> 0 under min_copy_num 1 changes nothing
    assert np.array_equal(lp[0], lp[2])
    exp = _expected_rescored(sg, base, changes, 1, rc, mp.arrays())
    assert np.array_equal(nres, exp.sum(axis=1))
    for c in range(3):
        assert np.array_equal(lp[c][exp[c]], lp_f[c][exp[c]])
        assert _close(lp[c], lp_f[c], 1e-9)
    assert _close(tot, tot_f, 1e-9 * len(reads))


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


def test_device_outputs_and_refusals(gpu_lib, diploid):
    sg, occ, param, reads, rc, mp = diploid
    base = sg.copy_num.astype(np.uint32)
    gm = D.PHMMModel(D.vectorised_to_phmm(sg, param, 0))
    rng = np.random.default_rng(8)
    chs = []
    for _ in range(5):
        ix = np.unique(rng.integers(0, base.size, size=16))
        chs.append((ix, base[ix] + 1))
    off, node, cn = _csr(base, chs)
    tot, lp, nres = gm.to_full_prob_reads_copy_num_changes(rc, mp, base, (off, node, cn), 0)
    dlp, dtot, dn = _DeviceArray(5 * len(reads)), _DeviceArray(5), _DeviceArray(5)
    L = _ffi.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def call(mph, b, n_c, o, nd, c, outs=(None, None, None)):
        return L.phmm_full_prob_reads_copy_num_changes(gm._h, rc._h, mph, None if b is None else p(b), 0, n_c,
                                                       None if o is None else p(o), p(nd), p(c), *outs)

    assert call(mp._h, base, 5, off, node, cn, (dlp.p, dtot.p, dn.p)) == _ffi.PHMM_OK
    assert np.array_equal(dlp.numpy().reshape(5, -1), lp) and np.array_equal(dtot.numpy(), tot)
    assert np.array_equal(dn.numpy(np.uint64), nres)
    # NULL outputs are fine; n_candidates = 0 writes nothing
    assert call(mp._h, base, 5, off, node, cn) == _ffi.PHMM_OK
    sentinel = np.full(3, 7.0)
    assert call(mp._h, base, 0, off, node, cn, (None, p(sentinel), None)) == _ffi.PHMM_OK
    assert np.all(sentinel == 7.0)
    # refusals, nothing written
    out = np.full(5, 7.0)
    bad_first = off.copy()
    bad_first[0] = 1
    decreasing = off.copy()
    decreasing[2] = decreasing[3] + 1
    big = node.copy()
    big[3] = base.size
    dup = node.copy()
    dup[1] = dup[0]
    other = D.ReadCollection(reads[:10])
    other_mp, _ = gm.generate_mappings(other, None, True)
    for args in ((None, base, off, node), (mp._h, None, off, node), (mp._h, base, bad_first, node),
                 (mp._h, base, decreasing, node), (mp._h, base, off, big), (mp._h, base, off, dup),
                 (other_mp._h, base, off, node), (mp._h, base, None, node)):
        assert call(args[0], args[1], 5, args[2], args[3], cn, (None, p(out), None)) == _ffi.PHMM_EINVAL
        assert np.all(out == 7.0)
    # node degree above 8 is refused as in the full form
    n = 12
    src = list(range(1, 11))
    dst = [0] * 10
    hub = D.SeqGraph(np.ones(n, dtype=np.int64), np.frombuffer(b"ACGTACGTACGT", dtype=np.uint8).copy(),
                     np.array(src, dtype=np.uint32), np.array(dst, dtype=np.uint32), None)
    hm = D.PHMMModel(D.vectorised_to_phmm(hub, D.PHMMParams.uniform(0.01).with_(n_warmup=2), 1))
    hr = D.ReadCollection([b"ACG"])
    hmp = D.Mappings.from_arrays(hr, np.arange(4, dtype=np.uint64), np.zeros(3, np.uint32), np.zeros(3))
    hb = np.ones(n, np.uint32)
    ho, hn, hc = _csr(hb, [([0], [2])])
    rcode = L.phmm_full_prob_reads_copy_num_changes(hm._h, hr._h, hmp._h, p(hb), 0, 1, p(ho), p(hn), p(hc), None,
                                                    p(out), None)
    assert rcode == _ffi.PHMM_EINVAL and np.all(out == 7.0)


def test_long_lists_reach_every_class(gpu_lib):
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
    tot_f, lp_f = gm.to_full_prob_reads_copy_nums(rc, mp, _materialise(base, changes), 0)
    tot, lp, nres = gm.to_full_prob_reads_copy_num_changes(rc, mp, base, changes, 0)
    exp = _expected_rescored(sg, base, changes, 0, rc, mp.arrays())
    assert np.array_equal(nres, exp.sum(axis=1))
    long_hit = exp & (read_max[None, :] > 128)
    assert long_hit.any() and (exp & (read_max[None, :] > 32) & (read_max[None, :] <= 64)).any() | long_hit.any()
    for c in range(len(chs)):
        assert np.array_equal(lp[c][exp[c]], lp_f[c][exp[c]]), c
        assert _close(lp[c], lp_f[c], 1e-9), c
    assert _close(tot, tot_f, 1e-9 * len(reads))
