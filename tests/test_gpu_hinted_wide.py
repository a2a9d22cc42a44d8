"""GPU: the wide class of the score-only hinted forward (hinted_wide_kernel.h): reads whose longest mapping list holds
65-400 nodes, one block per read and candidate group, in the full forms (phmm_full_prob_reads,
phmm_full_prob_reads_copy_nums, phmm_full_prob_reads_candidates), the change form and the likelihood handle.

Everything goes through the C ABI and is held to the oracle's full_prob_reads(reads, lists): 1e-9 per read, 1e-6 on
totals, every read compared.  The class is opt-in (PHMM_WIDE_HINTED=1, set for every test here); without it, or with
PHMM_NO_WIDE_HINTED=1, the generic one-wave kernels run.  The small numpy restatements
(materialised vectors, the rescored set) are those of test_gpu_copy_num_changes.py / test_gpu_likelihood.py (restated:
a test module cannot be imported without editing it)."""
import os

import numpy as np
import pytest

import dbgphmm_amd as D
from dbgphmm_amd import _ffi
from helpers import small_dbg_model

pytestmark = pytest.mark.gpu
K = 40
WIDTHS = (64, 65, 128, 129, 256, 257, 399, 400)
STATS_WIDE = 4


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


def _close(a, b, tol):
    a, b = np.asarray(a, float), np.asarray(b, float)
    both_inf = np.isneginf(a) & np.isneginf(b)
    with np.errstate(invalid="ignore"):
        return bool(np.all(both_inf | (np.abs(a - b) <= tol)))


def _maxdiff(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    with np.errstate(invalid="ignore"):
        d = np.where(np.isneginf(a) & np.isneginf(b), 0.0, np.abs(a - b))
    return float(np.max(d, initial=0.0))


def _read_max(rc, po):
    off, cnt = rc.offsets.astype(np.int64), np.diff(po.astype(np.int64))
    return np.array([cnt[off[r]:off[r + 1]].max() if off[r + 1] > off[r] else 0 for r in range(len(rc))])


# ------------------------------------------------------------------ 1. boundary widths on crafted lists
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
    om = oracle.Model(arrays)
    (po, nd, lp), _ = om.generate_mappings(reads, None, True, n_threads=8)
    plain = om.full_prob_reads(reads, (po, nd, lp), True, n_threads=8)
    ppo, pnd = pad_lists(po, nd, reads, arrays.n_nodes)
    want = om.full_prob_reads(reads, (ppo, pnd, np.zeros(pnd.size)), True, n_threads=8)
    assert np.all(np.isfinite(want)) and np.max(np.abs(want - plain)) < 1e-9  # (the padding is noise to the score)
    return arrays, reads, (ppo, pnd), want


def test_boundary_widths(gpu_lib, crafted):
    arrays, reads, (ppo, pnd), want = crafted
    assert arrays.n_nodes == 740 and len(reads) == 24
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    mp = D.Mappings.from_arrays(rc, ppo, pnd)
    rmax = _read_max(rc, ppo)
    assert sorted(set(rmax.tolist())) == sorted(WIDTHS)
    tot, lp = gm.to_full_prob_reads(rc, mp)
    launches, cells = _wide_stats()
    d = _maxdiff(lp, want)
    print(f"crafted widths: max |GPU - oracle| {d:.3e}, wide launches {launches}, cells {cells}")
    assert d <= 1e-9 and abs(tot - want.sum()) <= 1e-6
    assert launches > 0
    off = rc.offsets.astype(np.int64)
    wide = rmax > 64
    assert cells == int(sum(int(ppo[off[r + 1]]) - int(ppo[off[r]]) for r in np.flatnonzero(wide)))
    with _env("PHMM_NO_WIDE_HINTED"):
        tot_g, lp_g = gm.to_full_prob_reads(rc, mp)
        assert _wide_stats() == (0, 0)
    assert _maxdiff(lp_g, lp) <= 1e-9
    with _env("PHMM_WIDE_HINTED", "0"):  # not opted in: the generic kernels, the same bits as with the NO knob
        tot_d, lp_d = gm.to_full_prob_reads(rc, mp)
        assert _wide_stats() == (0, 0)
    assert np.array_equal(lp_d, lp_g)
    assert np.array_equal(lp_g[~wide], lp[~wide])  # lists of at most 64 nodes: the same kernel either way
    # the same bits on a second call
    assert np.array_equal(gm.to_full_prob_reads(rc, mp)[1], lp)


def test_duplicate_node_in_a_wide_list(gpu_lib, crafted):
    arrays, reads, _, _ = crafted
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads[:2])
    n = len(reads[0]) + len(reads[1])
    for width in (200, 100):  # the 448-thread and the 128-thread block
        lst = np.arange(width, dtype=np.uint32) + 7
        lst[width - 3] = lst[5]
        po = np.arange(n + 1, dtype=np.uint64) * width
        mp = D.Mappings.from_arrays(rc, po, np.tile(lst, n))
        with pytest.raises(D.PhmmError) as e:
            gm.to_full_prob_reads(rc, mp)
        assert e.value.code == _ffi.PHMM_EINVAL and "duplicate" in str(e.value)


# ------------------------------------------------------------------ 2.-4. natural wide lists on a tandem repeat
@pytest.fixture(scope="module")
def repeat(oracle):
    haps = D.tandem_repeat_polyploid_with_unique_homo_ends(20, 60, 0, 0.02, 0, 60, 2, 0.02, 0)
    sg = D.dbg_from_haplotypes(haps, K)
    param = D.PHMMParams.uniform(0.001).with_(n_warmup=K)
    reads = D.sample_genome_reads(haps, param, 20, 300, 0, 24)
    assert len(reads) == 24
    a1 = D.vectorised_to_phmm(sg, param, 1)
    lists, _ = oracle.Model(a1).generate_mappings(reads, None, True, n_threads=8)
    return sg, param, reads, lists


def _host_model(sg, param, vec, min_cn):
    with np.errstate(divide="ignore"):
        return D.vectorised_to_phmm(D.SeqGraph(np.asarray(vec, np.int64), sg.base, sg.edge_src, sg.edge_dst, None), param,
                                    min_cn)


def _oracle_scores(oracle, sg, param, reads, lists, vec, min_cn):
    return oracle.Model(_host_model(sg, param, vec, min_cn)).full_prob_reads(reads, lists, True, n_threads=8)


def _setup(repeat):
    sg, param, reads, lists = repeat
    rc = D.ReadCollection(reads)
    mp = D.Mappings.from_arrays(rc, *lists)
    return sg, param, reads, lists, rc, mp, _read_max(rc, lists[0])


def _batch(sg, rng, n):
    base = sg.copy_num.astype(np.uint32)
    out = [base.copy()]
    for _ in range(n - 1):
        v = base.copy()
        ix = np.unique(rng.integers(0, base.size, size=12))
        v[ix] = np.maximum(v[ix].astype(np.int64) + rng.choice([-1, 1], size=ix.size), 0)
        out.append(v)
    return np.array(out, np.uint32)


def test_natural_wide_lists(gpu_lib, oracle, repeat):
    sg, param, reads, lists, rc, mp, rmax = _setup(repeat)
    bands = [int(((rmax > lo) & (rmax <= hi)).sum()) for lo, hi in ((0, 64), (64, 128), (128, 256), (256, 400))]
    print("longest lists per read, bands <=64 / 65-128 / 129-256 / 257-400:", bands)
    assert bands[1] >= 2 and bands[2] >= 2 and sum(bands) == 24
    base = sg.copy_num.astype(np.uint32)
    gm = D.PHMMModel(_host_model(sg, param, base, 0))
    tot, lp = gm.to_full_prob_reads(rc, mp)
    assert _wide_stats()[0] > 0
    want = _oracle_scores(oracle, sg, param, reads, lists, base, 0)
    print(f"natural lists: max |GPU - oracle| {_maxdiff(lp, want):.3e}")
    assert _close(lp, want, 1e-9) and abs(tot - want.sum()) <= 1e-6
    cands = _batch(sg, np.random.default_rng(17), 9)
    for min_cn in (0, 1):
        tots, lps = gm.to_full_prob_reads_copy_nums(rc, mp, cands, min_cn)
        assert _wide_stats()[0] > 0
        for c in (3, 8):
            w = _oracle_scores(oracle, sg, param, reads, lists, cands[c], min_cn)
            print(f"batch min_cn {min_cn} candidate {c}: max |GPU - oracle| {_maxdiff(lps[c], w):.3e}")
            assert _close(lps[c], w, 1e-9) and abs(tots[c] - w.sum()) <= 1e-6
        for c in range(9):  # a batch is nine one-candidate calls, bit for bit
            t1, l1 = gm.to_full_prob_reads_copy_nums(rc, mp, cands[c:c + 1], min_cn)
            assert np.array_equal(l1[0], lps[c]) and t1[0] == tots[c], c
        for cpb in ("2", "4"):  # ... whatever number of candidates shares a block (9 = 2 x 4 + 1: idle slots too)
            with _env("PHMM_WIDE_HINTED_CPB", cpb):
                t2, l2 = gm.to_full_prob_reads_copy_nums(rc, mp, cands, min_cn)
            assert np.array_equal(l2, lps) and np.array_equal(t2, tots), cpb
        models = [_host_model(sg, param, v, min_cn) for v in cands]
        tp, lpp = gm.to_full_prob_reads_candidates(rc, mp, np.array([m.init_logp for m in models]),
                                                   np.array([m.trans_logp for m in models]))
        assert _close(lpp, lps, 1e-9) and _close(tp, tots, 1e-6)


def _find_cut(oracle, sg, param, reads, lists, base, base_lp):
    """a node whose copy number 0 cuts wide reads: the best node of base 200 of a read, read 5 first"""
    po, nd, _ = lists
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])])
    for r in [5] + [x for x in range(len(reads)) if x != 5]:
        if len(reads[r]) <= 200:
            continue
        v = int(nd[int(po[off[r] + 200])])
        vec = base.copy()
        vec[v] = 0
        lp = _oracle_scores(oracle, sg, param, reads, lists, vec, 0)
        victims = np.flatnonzero(np.isfinite(lp) & (base_lp - lp > 200.0))
        if victims.size >= 2:
            return vec, lp, victims
    raise AssertionError("no node cuts two reads")


def test_cut_reads_on_wide_lists(gpu_lib, oracle, repeat):
    sg, param, reads, lists, rc, mp, rmax = _setup(repeat)
    base = sg.copy_num.astype(np.uint32)
    base_lp = _oracle_scores(oracle, sg, param, reads, lists, base, 0)
    vec, want, victims = _find_cut(oracle, sg, param, reads, lists, base, base_lp)
    print("cut reads", victims.tolist(), "longest lists", rmax[victims].tolist(), "min", float(want[victims].min()))
    assert victims.size >= 2 and np.all(rmax[victims] > 64)
    gm = D.PHMMModel(_host_model(sg, param, base, 0))
    hm = _host_model(sg, param, vec, 0)

    def forms():
        a = gm.to_full_prob_reads_copy_nums(rc, mp, vec[None, :], 0)[1][0]
        b = gm.to_full_prob_reads_copy_num_changes(rc, mp, base, D.copy_num_changes(base, vec[None, :]), 0)[1][0]
        c = gm.to_full_prob_reads_candidates(rc, mp, hm.init_logp[None, :], hm.trans_logp[None, :])[1][0]
        return a, b, c

    for name, got in zip(("copy_nums", "changes", "candidates"), forms()):
        print(f"cut reads, {name}: max |GPU - oracle| {_maxdiff(got, want):.3e}")
        assert _close(got, want, 1e-9), name
    with _env("PHMM_NO_EXACT_HINTED"):
        for got in forms():
            assert np.all(np.isneginf(got[victims]))


def _csr(cand_changes):
    off = np.zeros(len(cand_changes) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(n) for n, _ in cand_changes])
    node = np.concatenate([np.asarray(n, np.uint32) for n, _ in cand_changes] + [np.zeros(0, np.uint32)])
    cn = np.concatenate([np.asarray(v, np.uint32) for _, v in cand_changes] + [np.zeros(0, np.uint32)])
    return off, node, cn


def _materialise(base, changes):
    off, node, cn = changes
    out = np.repeat(base[None, :], off.size - 1, axis=0)
    for c in range(off.size - 1):
        out[c, node[off[c]:off[c + 1]]] = cn[off[c]:off[c + 1]]
    return out


def _rescored(sg, base, changes, min_cn, rc, lists):
    """per candidate: the non-empty reads whose lists meet A_c = D_c + parents(D_c) (T_c and T_base stay above 0 here)"""
    po, nd, _ = lists
    off_r = rc.offsets.astype(np.int64)
    e_lo, e_hi = po[off_r[:-1]].astype(np.int64), po[off_r[1:]].astype(np.int64)
    eb = np.maximum(base.astype(np.int64), min_cn)
    off, node, cn = changes
    out = []
    for c in range(off.size - 1):
        ec = eb.copy()
        ec[node[off[c]:off[c + 1]].astype(np.int64)] = np.maximum(cn[off[c]:off[c + 1]].astype(np.int64), min_cn)
        dc = np.flatnonzero(ec != eb)
        a = np.zeros(base.size, bool)
        a[dc] = True
        a[sg.edge_src[np.isin(sg.edge_dst, dc)]] = True
        cum = np.concatenate([[0], np.cumsum(a[nd].astype(np.int64))])
        out.append((off_r[1:] > off_r[:-1]) & (cum[e_hi] > cum[e_lo]))
    return np.array(out)


def test_change_forms_and_handle(gpu_lib, repeat):
    sg, param, reads, lists, rc, mp, rmax = _setup(repeat)
    base = sg.copy_num.astype(np.uint32)
    R = len(reads)
    rng = np.random.default_rng(23)
    # 6 candidates of 1-4 node changes, on nodes the reads' lists hold
    listed = np.unique(lists[1])
    chs = []
    for n in (1, 2, 3, 4, 2, 1):
        ix = np.unique(rng.choice(listed, size=n, replace=False))
        chs.append((ix, np.maximum(base[ix].astype(np.int64) + rng.choice([-1, 1], size=ix.size), 1)))
    changes = _csr(chs)
    exp = _rescored(sg, base, changes, 0, rc, lists)
    assert (exp & (rmax[None, :] > 64)).any() and (~exp & (rmax[None, :] > 64)).any()
    gm = D.PHMMModel(_host_model(sg, param, base, 0))
    tot_f, lp_f = gm.to_full_prob_reads_copy_nums(rc, mp, _materialise(base, changes), 0)
    tot_s, lp_s, n_s = gm.to_full_prob_reads_copy_num_changes(rc, mp, base, changes, 0)
    assert _wide_stats()[0] > 0
    lk = gm.likelihood(rc, mp, base, 0)
    tot_h, lp_h, n_h = lk.score_changes(changes)
    assert _wide_stats()[0] > 0
    assert np.array_equal(n_s, exp.sum(axis=1)) and np.array_equal(n_h, n_s)
    for lp, tot in ((lp_s, tot_s), (lp_h, tot_h)):
        for c in range(exp.shape[0]):
            assert np.array_equal(lp[c][exp[c]], lp_f[c][exp[c]]), c  # rescored pairs: the bits of the full form
            assert _close(lp[c], lp_f[c], 1e-9), c
        assert _close(tot, tot_f, 1e-9 * R)
    # the same bits on a second call
    tot_s2, lp_s2, n_s2 = gm.to_full_prob_reads_copy_num_changes(rc, mp, base, changes, 0)
    tot_h2, lp_h2, n_h2 = lk.score_changes(changes)
    assert np.array_equal(lp_s2, lp_s) and np.array_equal(tot_s2, tot_s) and np.array_equal(n_s2, n_s)
    assert np.array_equal(lp_h2, lp_h) and np.array_equal(tot_h2, tot_h) and np.array_equal(n_h2, n_h)
    # ... and whatever number of pairs shares a block (work units with idle slots)
    for cpb in ("2", "4"):
        with _env("PHMM_WIDE_HINTED_CPB", cpb):
            tot_c, lp_c, n_c = gm.to_full_prob_reads_copy_num_changes(rc, mp, base, changes, 0)
            tot_k, lp_k, n_k = lk.score_changes(changes)
        assert np.array_equal(lp_c, lp_s) and np.array_equal(tot_c, tot_s) and np.array_equal(n_c, n_s), cpb
        assert np.array_equal(lp_k, lp_h) and np.array_equal(tot_k, tot_h) and np.array_equal(n_k, n_h), cpb
    # the generic kernels rescore the same pairs
    with _env("PHMM_NO_WIDE_HINTED"):
        tot_g, lp_g, n_g = gm.to_full_prob_reads_copy_num_changes(rc, mp, base, changes, 0)
        assert _wide_stats() == (0, 0)
    assert np.array_equal(n_g, n_s) and _close(lp_g, lp_s, 1e-9)
    # a chain of 5 moves: what the handle holds is the full form on the vector it holds
    vec = base.copy()
    for nodes, vals in chs[:5]:
        one = _csr([(nodes, vals)])
        hit = _rescored(sg, vec, one, 0, rc, lists)[0]
        tot, n = lk.move(np.asarray(nodes, np.uint32), np.asarray(vals, np.uint32))
        vec = _materialise(vec, one)[0]
        cur_cn, cur_lp, cur_tot = lk.current()
        assert np.array_equal(cur_cn, vec) and n == int(hit.sum())
        t1, l1 = gm.to_full_prob_reads_copy_nums(rc, mp, vec[None, :], 0)
        assert np.array_equal(cur_lp[hit], l1[0][hit])  # rescored reads: the same bits
        assert np.all(np.isfinite(cur_lp) == np.isfinite(l1[0]))
        assert _close(cur_lp, l1[0], 1e-9)
        assert _close(tot, t1[0], 1e-9 * R) and tot == cur_tot
