"""GPU: the promotion ladder of the score-only hinted forward (sparse.hip: hinted_run).  A read whose lists hold a
node with more in-list parents than its class has links per node is handed to the next generic class: <64, 2> ->
<128, 4> -> <400, 8>.  Only the generic kernels report link overflow, and they run for lists of at most 64 nodes only
where the lean kernels step aside, so the graph here has node degree 6.

42 nodes: a chain of 8, a bubble of 3 arms x 2 nodes and its join, a chain of 6, a bubble of 6 arms x 2 nodes and its
join, a chain of 8.  Every position of a read lists the same nodes: the first chain (no join: the read stays in
<64, 2>), the first 21 nodes (the 3-parent join: <128, 4>) or all 42 (the 6-parent join: <400, 8>).

Held to the oracle's full_prob_reads(reads, lists) at 1e-9 per read (the tolerance of test_gpu_hinted_wide.py); the
change form and the handle to the full form on the materialised vectors, bit for bit on the rescored pairs.  The
rescored set is restated in numpy as in test_gpu_copy_num_changes.py (restated: a test module cannot be imported
without editing it)."""
import numpy as np
import pytest

import dbgphmm_amd as D
from dbgphmm_amd import _ffi

pytestmark = pytest.mark.gpu
STATS_HINTED = 2
JOIN3, JOIN6 = 14, 33  # the joins of the two bubbles
N_FIRST = 21  # nodes up to the end of the second chain


def _graph():
    src, dst = [], []
    n = 0

    def chain(length, tail):
        nonlocal n
        for _ in range(length):
            if tail is not None:
                src.append(tail)
                dst.append(n)
            tail = n
            n += 1
        return tail

    def bubble(arms, tail):
        nonlocal n
        ends = []
        for _ in range(arms):
            src.extend([tail, n])
            dst.extend([n, n + 1])
            ends.append(n + 1)
            n += 2
        for e in ends:
            src.append(e)
            dst.append(n)
        n += 1
        return n - 1

    t = chain(8, None)
    t = bubble(3, t)
    assert t == JOIN3
    t = chain(6, t)
    assert n == N_FIRST
    t = bubble(6, t)
    assert t == JOIN6
    chain(8, t)
    assert n == 42
    rng = np.random.default_rng(11)
    base = np.array([b"ACGT"[int(rng.integers(0, 4))] for _ in range(n)], dtype=np.uint8)
    return D.SeqGraph(np.ones(n, dtype=np.int64), base, np.array(src, np.uint32), np.array(dst, np.uint32), None)


@pytest.fixture(scope="module")
def ladder(oracle):
    sg = _graph()
    assert np.bincount(sg.edge_dst, minlength=42).max() == 6 and np.bincount(sg.edge_src, minlength=42).max() == 6
    arrays = D.vectorised_to_phmm(sg, D.PHMMParams.uniform(0.01).with_(n_warmup=4), 1)
    drawn = D.sample_reads(arrays, 10 ** 9, 40, seed=4, max_reads=12)
    assert len(drawn) == 12
    reads, width = [], []
    for i, r in enumerate(drawn):
        reads.append((r[:6], r[:14], r)[i % 3])
        width.append((8, N_FIRST, 42)[i % 3])
    assert all(len(r) > 0 for r in reads)
    po = np.concatenate([[0], np.cumsum(np.repeat(width, [len(r) for r in reads]))]).astype(np.uint64)
    nd = np.concatenate([np.arange(w, dtype=np.uint32) for w, r in zip(width, reads) for _ in range(len(r))])
    want = oracle.Model(arrays).full_prob_reads(reads, (po, nd, np.zeros(nd.size)), True, n_threads=4)
    assert np.all(np.isfinite(want))
    return sg, arrays, reads, np.array(width), (po, nd), want


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
    po, nd = lists
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


def test_full_form_climbs_every_rung(gpu_lib, ladder):
    sg, arrays, reads, width, (po, nd), want = ladder
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    mp = D.Mappings.from_arrays(rc, po, nd)
    tot, lp = gm.to_full_prob_reads(rc, mp)
    _, launches, _ = _ffi.last_call_stats(STATS_HINTED)
    d = float(np.max(np.abs(lp - want)))
    print(f"promotion ladder: max |GPU - oracle| {d:.3e}, launches {launches}, ln P {want.min():.2f} .. {want.max():.2f}")
    assert d <= 1e-9
    # one launch per generic class: the 12 reads in <64, 2>, the 8 it flagged in <128, 4>, the 4 that flagged in
    # <400, 8>; no packed, wide or exact launch
    assert launches == 3
    assert np.array_equal(gm.to_full_prob_reads(rc, mp)[1], lp)  # the same bits on a second call


def test_change_form_and_handle_on_the_ladder(gpu_lib, ladder):
    sg, arrays, reads, width, (po, nd), want = ladder
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    mp = D.Mappings.from_arrays(rc, po, nd)
    base = np.ones(42, np.uint32)
    arm_end = int(sg.edge_src[np.flatnonzero(sg.edge_dst == JOIN6)[0]])
    chs = [([], []), ([JOIN3], [2]), ([arm_end], [2]), ([36, 37, 38], [2, 2, 2])]
    changes = _csr(chs)
    exp = _rescored(sg, base, changes, 1, rc, (po, nd))
    # nothing; the reads that list the first join; the reads that list everything, twice
    assert np.array_equal(exp[0], np.zeros(12, bool)) and np.array_equal(exp[1], width >= N_FIRST)
    assert np.array_equal(exp[2], width == 42) and np.array_equal(exp[3], width == 42)
    tot_f, lp_f = gm.to_full_prob_reads_copy_nums(rc, mp, _materialise(base, changes), 1)
    assert float(np.max(np.abs(lp_f[0] - want))) <= 1e-9
    tot, lp, nres = gm.to_full_prob_reads_copy_num_changes(rc, mp, base, changes, 1)
    assert np.array_equal(nres, exp.sum(axis=1)), (nres, exp.sum(axis=1))
    for c in range(4):
        assert np.array_equal(lp[c][exp[c]], lp_f[c][exp[c]]), c  # rescored pairs: the bits of the full form
        assert float(np.max(np.abs(lp[c] - lp_f[c]))) <= 1e-9, c
    # the handle's batch: the change form's bits
    lk = gm.likelihood(rc, mp, base, 1)
    tot_h, lp_h, n_h = lk.score_changes(changes)
    assert np.array_equal(n_h, nres) and np.array_equal(lp_h, lp)
    assert float(np.max(np.abs(tot_h - tot))) <= 1e-9 * len(reads)  # (the handle sums on the device, over a tree)
