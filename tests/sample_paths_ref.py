"""Posterior path sampling over mapping lists in plain Python (test infrastructure, imported like best_path_ref.py):
the restatement phmm_run_with_mapping_sample_paths is held to -- the forward sums, the random stream, the draw rule
and the walk back exactly as include/phmm_amd_sample.h writes them -- and the fixtures the CPU and the GPU tests share.

The forward pass is the recursion of include/phmm_amd_path.h with every maximum replaced by a log-sum-exp over the same
candidates in the same order (lse below).  A node listed twice holds states at its first entry only; the later entries
are -inf everywhere.  The walk consumes one draw per decision, a decision with one candidate included; InsBegin has one
predecessor and consumes none.

draw() also returns the decision's margin: the distance of u * c_last to the nearest inner boundary of the running
sums, divided by c_last.  The device's exp / log and Python's may differ in the last bits of the forward values, so the
rows of the two sides can be compared word for word only where no decision lies that close to a boundary; the CPU test
asserts it of every shared fixture (a condition on the inputs, not a tolerance on the result).

Parallel edges.  The rows do not say which of two edges u -> v a step took, and score_path re-scores a step over the
heavier one.  A walk that took the lighter edge therefore has own terms that sum to score_path's value plus
(t_taken - t_heavier); the walk returns that correction per sample (0.0 exactly where no such step occurs)."""
import functools
import math

import numpy as np

import best_path_ref as B
from best_path_ref import (INS_BEGIN, NINF, NONE, IllegalPath, bar, csr, full_lists, linear, lists_of,  # noqa: F401
                           many_short_reads, odd_cases, pad_unreachable, score_path, shift_slots, with_isolated)
from graph_cases import base_case

MASK64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15
MAX_SAMPLES = 64
MIN_MARGIN = 1e-9  # the condition item 4 of the issue puts on every fixture compared word for word


# ---------------------------------------------------------------- the random stream
def mix(z):
    """the SplitMix64 finaliser"""
    z &= MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def stream(seed, r, s):
    """x0 of read r (its index in the read set) and sample s"""
    return mix((seed & MASK64) ^ mix((r * 64 + s + GOLD) & MASK64))


def uniform(x0, d):
    """draw d = 1, 2, .. of a stream, in [0, 1)"""
    return (mix((x0 + d * GOLD) & MASK64) >> 11) * 2.0 ** -53


# ---------------------------------------------------------------- the sums and the draw rule
def lse(terms):
    """mx + ln sum exp(t - mx) over the terms in their order; -inf terms add 0; -inf without a finite term"""
    mx = NINF
    for t in terms:
        if t > mx:
            mx = t
    if mx == NINF:
        return NINF
    s = 0.0
    for t in terms:
        s += math.exp(t - mx) if t > NINF else 0.0
    return mx + math.log(s)


def weights(terms):
    """-> (mx, [w_i]) of the draw rule; all zeros when no term is finite"""
    mx = NINF
    for t in terms:
        if t > mx:
            mx = t
    if mx == NINF:
        return mx, [0.0] * len(terms)
    return mx, [math.exp(t - mx) if t > NINF else 0.0 for t in terms]


def draw(terms, u):
    """the draw rule of the header -> (choice, margin); choice is None when no term is finite"""
    _, w = weights(terms)
    c, run = [], 0.0
    for x in w:
        run += x
        c.append(run)
    if not run > 0.0:
        return None, math.inf
    thr = u * run
    choice = None
    for i, ci in enumerate(c):
        if thr < ci:
            choice = i
            break
    if choice is None:
        choice = max(i for i, x in enumerate(w) if x > 0.0)
    margin = math.inf
    for ci in c:
        if 0.0 < ci < run:
            margin = min(margin, abs(thr - ci) / run)
    return choice, margin


# ---------------------------------------------------------------- the forward sums
class Forward:
    """what the walk reads: per position the list, M, I, D, the Del levels, the first-entry slots of every parent in the
    previous and in the same list (ascending edge index), the node's own first entry in the previous list, and InsBegin"""
    __slots__ = ("L", "G", "cols", "ib", "logz", "end_terms")


def _edges_in(arrays):
    """node -> [(parent, trans_logp), ...] in ascending edge index (parallel edges stay apart)"""
    return B._parents(arrays)


def forward(arrays, read, lists):
    p = arrays.param
    G, L = int(p.n_max_gaps), len(read)
    par, emis, init = _edges_in(arrays), arrays.emission.tolist(), arrays.init_logp.tolist()
    F = Forward()
    F.L, F.G, F.cols, F.ib = L, G, [], []
    pslot, pM, pI, pD = {}, [], [], []
    ib = NINF
    for pos in range(L):
        nodes = [int(v) for v in lists[pos]]
        n, x = len(nodes), read[pos]
        slot = {}
        for j, v in enumerate(nodes):
            slot.setdefault(v, j)
        first = [slot[v] == j for j, v in enumerate(nodes)]
        beg_m = p.p_MM if pos == 0 else p.p_IM + ib
        M, I = [NINF] * n, [NINF] * n
        prev_par = [[(pslot[u], t) for u, t in par[v] if u in pslot] if first[j] else [] for j, v in enumerate(nodes)]
        same_par = [[(slot[u], t) for u, t in par[v] if u in slot] if first[j] else [] for j, v in enumerate(nodes)]
        me = [pslot.get(v) if first[j] else None for j, v in enumerate(nodes)]
        for j, v in enumerate(nodes):
            if not first[j]:
                continue
            terms = []
            for q, t in prev_par[j]:
                terms += [t + (p.p_MM + pM[q]), t + (p.p_IM + pI[q]), t + (p.p_DM + pD[q])]
            terms.append(init[v] + beg_m)
            M[j] = (p.p_match if emis[v] == x else p.p_mismatch) + lse(terms)
            q = me[j]
            if q is not None:
                I[j] = p.p_random + lse([p.p_MI + pM[q], p.p_II + pI[q], p.p_DI + pD[q]])
        ib = p.p_random + (p.p_MI if pos == 0 else p.p_II + ib)
        beg_d = p.p_ID + ib
        lev = [[NINF] * n]
        for j, v in enumerate(nodes):
            if not first[j]:
                continue
            terms = []
            for q, t in same_par[j]:
                terms += [t + (p.p_MD + M[q]), t + (p.p_ID + I[q])]
            terms.append(init[v] + beg_d)
            lev[0][j] = lse(terms)
        for t_ in range(1, G + 1):
            nx = [NINF] * n
            for j in range(n):
                if first[j]:
                    nx[j] = lse([t + (p.p_DD + lev[t_ - 1][q]) for q, t in same_par[j]])
            lev.append(nx)
        Dv = [lse([lev[t_][j] for t_ in range(G + 1)]) if first[j] else NINF for j in range(n)]
        F.cols.append(dict(nodes=nodes, M=M, I=I, D=Dv, lev=lev, prev_par=prev_par, same_par=same_par, me=me))
        F.ib.append(ib)
        pslot, pM, pI, pD = slot, M, I, Dv
    F.end_terms = [x for j in range(len(pM)) for x in (pM[j], pI[j], pD[j])]
    F.logz = p.p_end + lse(F.end_terms) if L else NINF
    return F


# ---------------------------------------------------------------- the walk
def walk(arrays, read, F, x0, log=None):
    """one sampled path -> (rows[L, G + 2], ln P from the walk's own terms, counts[4], smallest margin, correction for
    lighter parallel edges); log, if a list, receives (pos, what, choice, margin) per decision.  Call only when
    F.logz > -inf."""
    p = arrays.param
    G, L = F.G, F.L
    emis, init = arrays.emission.tolist(), arrays.init_logp.tolist()
    edge_max = getattr(arrays, "_sample_paths_heavy", None)
    if edge_max is None:
        edge_max = {}
        for u, v, t in zip(arrays.edge_src.tolist(), arrays.edge_dst.tolist(), arrays.trans_logp.tolist()):
            edge_max[(u, v)] = max(t, edge_max.get((u, v), NINF))
        arrays._sample_paths_heavy = edge_max
    rows = np.full((L, G + 2), NONE, dtype=np.uint32)
    cnt = [0, 0, 0, 0]
    state = {"d": 0, "margin": math.inf, "corr": 0.0}

    def decide(terms, pos, what):
        state["d"] += 1
        c, mg = draw(terms, uniform(x0, state["d"]))
        if c is None:
            raise AssertionError(f"base {pos}: a decision ({what}) without a finite candidate")
        state["margin"] = min(state["margin"], mg)
        if log is not None:
            log.append((pos, what, c, mg))
        return c

    def lighter(u, v, t):
        if t > NINF:
            state["corr"] += t - edge_max[(u, v)]

    c = decide(F.end_terms, L - 1, "end")
    st = (c // 3, c % 3)  # (slot, kind) in column pos, or "IB" = InsBegin of column pos
    acc = p.p_end
    for pos in range(L - 1, -1, -1):
        col = F.cols[pos]
        nodes = col["nodes"]
        if st != "IB" and st[1] == 2:
            j = st[0]
            t_ = decide([col["lev"][t][j] for t in range(G + 1)], pos, "level")
            while True:
                rows[pos, t_ + 1] = (j << 2) | 2
                cnt[3] += 1
                if t_ == 0:
                    break
                cand = col["same_par"][j]
                c = decide([t + (p.p_DD + col["lev"][t_ - 1][q]) for q, t in cand], pos, "parent")
                q, t = cand[c]
                acc += t + p.p_DD
                lighter(nodes[q], nodes[j], t)
                j, t_ = q, t_ - 1
            cand = col["same_par"][j]
            terms = []
            for q, t in cand:
                terms += [t + (p.p_MD + col["M"][q]), t + (p.p_ID + col["I"][q])]
            terms.append(init[nodes[j]] + (p.p_ID + F.ib[pos]))
            c = decide(terms, pos, "level 0")
            if c == len(terms) - 1:
                acc += init[nodes[j]] + p.p_ID
                st = "IB"
            else:
                q, t = cand[c // 2]
                acc += t + (p.p_MD if c % 2 == 0 else p.p_ID)
                lighter(nodes[q], nodes[j], t)
                st = (q, c % 2)
        if st == "IB":
            rows[pos, 0] = INS_BEGIN
            cnt[2] += 1
            acc += p.p_random + (p.p_MI if pos == 0 else p.p_II)
        elif st[1] == 0:
            j = st[0]
            v = nodes[j]
            rows[pos, 0] = (j << 2) | 0
            hit = emis[v] == read[pos]
            cnt[0 if hit else 1] += 1
            acc += p.p_match if hit else p.p_mismatch
            cand = col["prev_par"][j]
            prev = F.cols[pos - 1] if pos else None
            terms = []
            for q, t in cand:
                terms += [t + (p.p_MM + prev["M"][q]), t + (p.p_IM + prev["I"][q]), t + (p.p_DM + prev["D"][q])]
            terms.append(init[v] + (p.p_MM if pos == 0 else p.p_IM + F.ib[pos - 1]))
            c = decide(terms, pos, "match")
            if c == len(terms) - 1:
                acc += init[v] + (p.p_MM if pos == 0 else p.p_IM)
                st = "IB"
            else:
                q, t = cand[c // 3]
                acc += t + (p.p_MM, p.p_IM, p.p_DM)[c % 3]
                lighter(prev["nodes"][q], v, t)
                st = (q, c % 3)
        else:
            j = st[0]
            rows[pos, 0] = (j << 2) | 1
            cnt[2] += 1
            acc += p.p_random
            q = col["me"][j]
            prev = F.cols[pos - 1]
            c = decide([p.p_MI + prev["M"][q], p.p_II + prev["I"][q], p.p_DI + prev["D"][q]], pos, "ins")
            acc += (p.p_MI, p.p_II, p.p_DI)[c]
            st = (q, c)
    assert st == "IB", st
    return rows, acc, cnt, state["margin"], state["corr"]


def sample_read(arrays, read, lists, r, n_samples, seed, F=None, logs=None):
    """the call's outputs for one read with index r in its read set
    -> dict(logz, path_logp[S], rows[S, L, G + 2], counts[S, 4], margin, corr[S])"""
    F = forward(arrays, read, lists) if F is None else F
    S, L, G = n_samples, len(read), F.G
    out = dict(logz=F.logz, path_logp=np.full(S, NINF), rows=np.full((S, L, G + 2), NONE, dtype=np.uint32),
               counts=np.zeros((S, 4), dtype=np.uint32), margin=math.inf, corr=np.zeros(S))
    if not F.logz > NINF:
        return out
    for s in range(S):
        log = None if logs is None else logs.setdefault(s, [])
        rows, acc, cnt, mg, corr = walk(arrays, read, F, stream(seed, r, s), log)
        out["rows"][s], out["path_logp"][s], out["counts"][s], out["corr"][s] = rows, acc, cnt, corr
        out["margin"] = min(out["margin"], mg)
    return out


def sample_set(arrays, reads, lists, n_samples, seed):
    """every read of a read set -> [sample_read(...)]; equal (read, lists) pairs share one forward pass"""
    cache, out = {}, []
    for r, (read, ls) in enumerate(zip(reads, lists)):
        key = (bytes(read), repr(ls))
        if key not in cache:
            cache[key] = forward(arrays, read, ls)
        out.append(sample_read(arrays, read, ls, r, n_samples, seed, cache[key]))
    return out


def first_difference(arrays, read, lists, r, s, seed, rows):
    """where the walk of (r, s) departs from `rows` -> text: the first decision (the walk goes backwards) whose base has
    another row, and its margin"""
    logs = {}
    F = forward(arrays, read, lists)
    rows_ref, *_ = walk(arrays, read, F, stream(seed, r, s), logs.setdefault(s, []))
    bad = np.flatnonzero((np.asarray(rows) != rows_ref).any(axis=1))
    if bad.size == 0:
        return "no difference"
    g = int(bad[-1])
    at = [d for d in logs[s] if d[0] == g] or [d for d in logs[s] if d[0] == g + 1][-1:]
    return (f"read {r} sample {s}: base {g} has {np.asarray(rows)[g].tolist()} for {rows_ref[g].tolist()}; decisions there "
            + ", ".join(f"{w} -> {c} (margin {m:.3e})" for _, w, c, m in at))


def usage_of(rows_plane, reads, lists, n_nodes):
    """the host recount of out_node_usage from one plane of out_path: Match, Ins and Del states per node"""
    use = np.zeros(n_nodes, dtype=np.uint32)
    g = 0
    for read, ls in zip(reads, lists):
        for i in range(len(read)):
            for c in rows_plane[g + i].tolist():
                if c not in (NONE, INS_BEGIN):
                    use[ls[i][c >> 2]] += 1
        g += len(read)
    return use


# ---------------------------------------------------------------- chi-square of sampled paths against the exact law
CHI_READS = (b"ATTCGTCGT", b"ATTCA")
CHI_COPIES, CHI_SAMPLES, CHI_SEED = 625, 64, 7


def chi_case():
    arrays = linear(0.1)
    return arrays, CHI_READS


def chi_square(arrays, read, lists, logz, walks):
    """walks: the rows of N sampled paths of one read -> (chi-square, df, distinct paths).  Cells: every distinct path
    whose expectation N exp(value - ln Z) is >= 5; all other paths, unseen mass included, in one cell."""
    N = len(walks)
    seen = {}
    for rows in walks:
        key = np.asarray(rows, dtype=np.uint32).tobytes()
        if key not in seen:
            seen[key] = [0, rows]
        seen[key][0] += 1
    chi, cells, big_n, big_e = 0.0, 0, 0, 0.0
    for count, rows in seen.values():
        value, _, _ = score_path(arrays, read, lists, rows)
        e = N * math.exp(value - logz)
        if e >= 5.0:
            chi += (count - e) ** 2 / e
            cells += 1
            big_n += count
            big_e += e
    rest_e = N - big_e
    if rest_e > 0.0:
        chi += ((N - big_n) - rest_e) ** 2 / rest_e
        cells += 1
    return chi, cells - 1, len(seen)


def chi_bar(df):
    return df + 5.0 * math.sqrt(2.0 * df)


# ---------------------------------------------------------------- the fixtures compared word for word
def _oracle_lists(arrays, reads):
    po, nd, _ = B._oracle_lists(arrays, reads)
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])])
    return [lists_of(po, nd, int(off[j]), int(off[j + 1])) for j in range(len(reads))]


@functools.lru_cache(maxsize=None)
def graph_fixture(graph):
    """base_case(graph): its 12 reads cut to 40 bases, lists from generate_mappings (the oracle's, so that the CPU and the
    GPU tests walk the same lists)"""
    b = base_case(graph)
    reads = [r[:40] for r in b["reads"]]
    return dict(tag=graph, arrays=b["arrays"], reads=reads, lists=_oracle_lists(b["arrays"], reads), n_samples=64,
                seed=SEEDS[graph])


@functools.lru_cache(maxsize=None)
def linear_fixture():
    arrays = linear(0.01)
    reads = [b"ATTCGTCGT", b"ATTCGCATCGT", b"ATTCGATGGT"]
    return dict(tag="linear mock, uniform(0.01)", arrays=arrays, reads=reads, lists=[full_lists(arrays, r) for r in reads],
                n_samples=64, seed=SEEDS["linear"])


# one seed per fixture; a fixture that fails the margin condition gets another seed here (never another threshold)
SEEDS = {"dbg": 11, "zoo": 12, "linear": 13, "odd": 14, "consistency": 15}


@functools.lru_cache(maxsize=None)
def fixtures():
    """-> [dict(tag, arrays, reads, lists[read][pos], n_samples, seed)]: dbg, zoo, the linear mock with errors, and every
    group of odd_cases("ord") at n_samples = 3"""
    out = [graph_fixture("dbg"), graph_fixture("zoo"), linear_fixture()]
    for g in odd_cases("ord"):
        out.append(dict(tag=g["tag"], arrays=g["arrays"], reads=g["reads"], lists=g["lists"], n_samples=3, seed=SEEDS["odd"]))
    return out


@functools.lru_cache(maxsize=None)
def fixture_samples(k):
    f = fixtures()[k]
    return sample_set(f["arrays"], f["reads"], f["lists"], f["n_samples"], f["seed"])


CONSISTENCY_COPIES = 16


@functools.lru_cache(maxsize=None)
def consistency_case():
    """dbg with 16 copies of each read one after the other (copy c of read j has index j * 16 + c)"""
    f = graph_fixture("dbg")
    reads = [r for r in f["reads"] for _ in range(CONSISTENCY_COPIES)]
    lists = [ls for ls in f["lists"] for _ in range(CONSISTENCY_COPIES)]
    return dict(tag="dbg x 16", arrays=f["arrays"], reads=reads, lists=lists, n_samples=64, seed=SEEDS["consistency"])


def emitting_frequencies(rows_by_copy, L, n_entries):
    """rows_by_copy: [copies][S, L, stride] -> freq[L][slot][kind 0 / 1]: the share of the walks whose base p is emitted
    by Match / Ins of the slot"""
    freq = [np.zeros((n_entries[p], 2)) for p in range(L)]
    n = 0
    for planes in rows_by_copy:
        for rows in planes:
            n += 1
            for p in range(L):
                c = int(rows[p, 0])
                if c not in (NONE, INS_BEGIN):
                    freq[p][c >> 2, c & 3] += 1
    return [f / n for f in freq], n


def binomial_bar(prob, n):
    """6 binomial standard deviations plus 1 / N"""
    return 6.0 * math.sqrt(max(prob * (1.0 - prob), 0.0) / n) + 1.0 / n
