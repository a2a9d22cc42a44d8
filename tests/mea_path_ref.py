"""The weighted walk over mapping lists in Python (test infrastructure, imported like best_path_ref.py): the
restatement of include/phmm_amd_mea.h that phmm_run_with_mapping_weighted_path -- and through it the MEA call -- is held
to bit for bit, and a scorer of any path in the out_path encoding under given weights.

The path family, the ranks and the rows are those of best_path_ref.py.  What changes is what the numbers mean: the
model's logs only say which transitions are admissible (the term the best-path recursion would add is > -inf); the
value of a state is fl(largest admissible source value + own weight), one double addition, so a path is worth its
weights summed left to right.  `w` is [n_entries_of_the_read, 3] (Match, Ins, Del per entry, entries in list order,
position after position), `ib` one weight per base or None."""
import math

import numpy as np

import best_path_ref as B
from best_path_ref import INS_BEGIN, NINF, NONE, IllegalPath, _BEGIN, _parents, _take


def _via(term, v):
    """the source's value if the transition exists"""
    return v if term > NINF else NINF


def entry_offsets(lists):
    off = [0]
    for lst in lists:
        off.append(off[-1] + len(lst))
    return off


def weighted_path_ref(arrays, read, lists, w, ib=None):
    """-> (score, rows): the largest left-to-right weight sum over the legal paths of `read` over `lists` and the path
    the tie rule leaves, as rows[L, n_max_gaps + 2] in the out_path encoding (all NONE when the score is -inf)"""
    p = arrays.param
    G, L = int(p.n_max_gaps), len(read)
    par, emis, init = _parents(arrays), arrays.emission.tolist(), arrays.init_logp.tolist()
    rows = np.full((L, G + 2), NONE, dtype=np.uint32)
    if L == 0:
        return NINF, rows
    w = np.asarray(w, dtype=np.float64).reshape(-1, 3).tolist()
    ibw = [0.0] * L if ib is None else np.asarray(ib, dtype=np.float64).tolist()
    eoff = entry_offsets(lists)
    assert len(w) == eoff[-1] and len(ibw) == L
    emit_i = p.p_random > NINF
    pslot, pM, pI, pD = {}, [], [], []
    ibv = NINF
    back = []  # per position: (srcM, srcI, slotI, lvlD, srcD0, parD[t][j])
    for pos in range(L):
        nodes = [int(v) for v in lists[pos]]
        n, x, wp = len(nodes), read[pos], w[eoff[pos]:eoff[pos + 1]]
        slot = {}
        for j, v in enumerate(nodes):
            slot.setdefault(v, j)
        beg_v, beg_t = (0.0, p.p_MM) if pos == 0 else (ibv, p.p_IM)
        M, I, srcM, srcI, slotI = [NINF] * n, [NINF] * n, [_BEGIN] * n, [0] * n, [0] * n
        for j, v in enumerate(nodes):
            b, r = NINF, _BEGIN + 1
            for u, t in par[v]:
                q = pslot.get(u)
                if q is None:
                    continue
                b, r = _take(b, r, _via(t + p.p_MM, pM[q]), (q << 2) | 0)
                b, r = _take(b, r, _via(t + p.p_IM, pI[q]), (q << 2) | 1)
                b, r = _take(b, r, _via(t + p.p_DM, pD[q]), (q << 2) | 2)
            b, r = _take(b, r, _via(init[v] + beg_t, beg_v), _BEGIN)
            M[j], srcM[j] = _via(p.p_match if emis[v] == x else p.p_mismatch, b) + wp[j][0], r
            q = pslot.get(v)
            if q is not None and emit_i:
                b, r = NINF, 4
                b, r = _take(b, r, _via(p.p_MI, pM[q]), 0)
                b, r = _take(b, r, _via(p.p_II, pI[q]), 1)
                b, r = _take(b, r, _via(p.p_DI, pD[q]), 2)
                I[j], srcI[j], slotI[j] = b + wp[j][1], r, q
        ibv = (_via(p.p_MI, 0.0) if pos == 0 else _via(p.p_II, ibv)) + ibw[pos] if emit_i else NINF
        inlist = [[(slot[u], t) for u, t in par[v] if u in slot] for v in nodes]
        lv, srcD0 = [NINF] * n, [_BEGIN] * n
        for j, v in enumerate(nodes):
            b, r = NINF, _BEGIN + 1
            for q, t in inlist[j]:
                b, r = _take(b, r, _via(t + p.p_MD, M[q]), (q << 1) | 0)
                b, r = _take(b, r, _via(t + p.p_ID, I[q]), (q << 1) | 1)
            b, r = _take(b, r, _via(init[v] + p.p_ID, ibv), _BEGIN)
            lv[j], srcD0[j] = b + wp[j][2], r
        Dv, lvlD, parD = list(lv), [0] * n, [None]
        for t_ in range(1, G + 1):
            nx, pr = [NINF] * n, [0] * n
            for j in range(n):
                b, r = NINF, _BEGIN
                for q, t in inlist[j]:
                    b, r = _take(b, r, _via(t + p.p_DD, lv[q]), q)
                nx[j], pr[j] = b + wp[j][2], r
                if nx[j] > Dv[j]:
                    Dv[j], lvlD[j] = nx[j], t_
            parD.append(pr)
            lv = nx
        back.append((srcM, srcI, slotI, lvlD, srcD0, parD))
        pslot, pM, pI, pD = slot, M, I, Dv
    b, r = NINF, _BEGIN
    if p.p_end > NINF:
        for j in range(len(pM)):
            b, r = _take(b, r, pM[j], (j << 2) | 0)
            b, r = _take(b, r, pI[j], (j << 2) | 1)
            b, r = _take(b, r, pD[j], (j << 2) | 2)
    if not b > NINF:
        return NINF, rows
    state = r  # (slot << 2) | kind in column pos, or _BEGIN = InsBegin of column pos
    for pos in range(L - 1, -1, -1):
        srcM, srcI, slotI, lvlD, srcD0, parD = back[pos]
        if state != _BEGIN and state & 3 == 2:
            j = state >> 2
            T = lvlD[j]
            for t_ in range(T, -1, -1):
                rows[pos, t_ + 1] = (j << 2) | 2
                if t_:
                    j = parD[t_][j]
            s0 = srcD0[j]
            state = _BEGIN if s0 == _BEGIN else ((s0 >> 1) << 2) | (s0 & 1)
        if state == _BEGIN:
            rows[pos, 0] = INS_BEGIN
        else:
            rows[pos, 0] = state
            j = state >> 2
            state = srcM[j] if state & 3 == 0 else (slotI[j] << 2) | srcI[j]
    return b, rows


def score_rows(arrays, read, lists, rows, w, ib=None):
    """the weights of a path given in the out_path encoding, summed from base 0 in path order (the emitting state, then
    each Del in the order passed), one double addition per state -> (score, counts[4]); raises IllegalPath if the rows
    are no path of the model over these lists (best_path_ref.score_path decides) or take a transition of probability 0"""
    logp, _, counts = B.score_path(arrays, read, lists, rows)
    if not logp > NINF:
        raise IllegalPath("the path takes a transition or an emission of probability 0")
    w = np.asarray(w, dtype=np.float64).reshape(-1, 3).tolist()
    eoff = entry_offsets(lists)
    total = 0.0
    for pos, row in enumerate(np.asarray(rows).tolist()):
        for c in row:
            if c == NONE:
                break
            total = total + ((0.0 if ib is None else float(ib[pos])) if c == INS_BEGIN else w[eoff[pos] + (c >> 2)][c & 3])
    return total, counts


def counts_of(arrays, read, lists, rows):
    """matches, mismatches, insertions, deletions read off the rows (zeros for a read without a path)"""
    emis, cnt = arrays.emission.tolist(), [0, 0, 0, 0]
    for pos, row in enumerate(np.asarray(rows).tolist()):
        for c in row:
            if c == NONE:
                break
            if c == INS_BEGIN or c & 3 == 1:
                cnt[2] += 1
            elif c & 3 == 2:
                cnt[3] += 1
            else:
                cnt[0 if emis[int(lists[pos][c >> 2])] == read[pos] else 1] += 1
    return cnt


def check_read(arrays, read, lists, w, ib, score, rows, counts):
    """what every parity test asks of one read's outputs: score equal as a double, rows and counts word for word -> the
    restatement's score"""
    want, ref_rows = weighted_path_ref(arrays, read, lists, w, ib)
    rows = np.asarray(rows)
    assert score == want, (score, want)
    if not np.array_equal(rows, ref_rows):
        g = int(np.flatnonzero((rows != ref_rows).any(axis=1))[-1])  # the walk goes backwards: the last row departs first
        raise AssertionError(f"the path departs from the restatement's at base {g}: {rows[g].tolist()} for {ref_rows[g].tolist()}")
    assert list(counts) == counts_of(arrays, read, lists, ref_rows), (list(counts), ref_rows)
    if want > NINF:
        got, cnt = score_rows(arrays, read, lists, rows, w, ib)
        assert got == want and cnt == list(counts), (got, want, cnt, list(counts))
    else:
        assert np.all(rows == NONE) and list(counts) == [0, 0, 0, 0]
    return want


def dyadic(rng, shape, lo=-1, hi=4):
    """random multiples of 1/4 (of 2^-10 a fortiori: their sums are exact, so equal paths tie exactly); a few values
    only, so that they do"""
    return rng.integers(lo, hi, size=shape).astype(np.float64) / 4.0
