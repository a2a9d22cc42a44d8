"""The best path over mapping lists in numpy and Python (test infrastructure, imported like fuzz_cases.py): the
definition that phmm_run_with_mapping_best_path is held to, a scorer of any path in the out_path encoding, and the
cases the CPU and the GPU tests share.

The recursion is forward_with_mapping (forward.rs:51-75, f_step 276-306) with every sum replaced by a maximum, in natural
logs (include/phmm_amd_path.h has it in full).  `lists` is one sequence of node ids per read position.  A node listed
twice is looked up at its first entry.  Ties go by the header's rule: the lower rank wins among exactly equal values.

The bar.  A path value is a sum of n_terms non-positive terms, so any order of summation is off by at most
(n_terms - 1) u |ln P| to first order, u = 2^-53; two evaluations double it; the last factor 2 covers second order:
bar = 4 n_terms 2^-53 |ln P|."""
import functools
import math

import numpy as np

import dbgphmm_amd as D
from fuzz_cases import make_case
from graph_cases import base_case
from helpers import small_dbg_model
from repeat_cases import dataset

NONE = 0xFFFFFFFF
INS_BEGIN = 0xFFFFFFFD
NINF = -math.inf
_BEGIN = 1 << 30  # rank of Begin / InsBegin: behind every node state


def bar(n_terms, logp):
    return 4.0 * n_terms * 2.0 ** -53 * abs(logp)


def _parents(arrays):
    """node -> [(parent, trans_logp), ...], one entry per edge (parallel edges stay apart)"""
    par = getattr(arrays, "_best_path_parents", None)
    if par is None:
        par = [[] for _ in range(arrays.n_nodes)]
        for u, v, t in zip(arrays.edge_src.tolist(), arrays.edge_dst.tolist(), arrays.trans_logp.tolist()):
            par[v].append((u, t))
        arrays._best_path_parents = par
    return par


def lists_of(po, nd, g0, g1):
    """the lists of the positions g0..g1-1 of a CSR (pos_off, nodes)"""
    return [nd[int(po[g]):int(po[g + 1])].tolist() for g in range(g0, g1)]


def _take(best, rank, v, r):
    return (v, r) if v > best or (v == best and v > NINF and r < rank) else (best, rank)


def best_path_ref(arrays, read, lists):
    """-> (best, rows): ln P of the best path of `read` over `lists` and the path as rows[L, n_max_gaps + 2] in the
    out_path encoding (all NONE when best is -inf)"""
    p = arrays.param
    G, L = int(p.n_max_gaps), len(read)
    stride = G + 2
    par, emis, init = _parents(arrays), arrays.emission.tolist(), arrays.init_logp.tolist()
    rows = np.full((L, stride), NONE, dtype=np.uint32)
    if L == 0:
        return NINF, rows
    pslot, pM, pI, pD = {}, [], [], []
    ib = NINF
    back = []  # per position: (srcM, srcI, slotI, lvlD, srcD0, parD[t][j])
    for pos in range(L):
        nodes = [int(v) for v in lists[pos]]
        n, x = len(nodes), read[pos]
        slot = {}
        for j, v in enumerate(nodes):
            slot.setdefault(v, j)
        beg_m = p.p_MM if pos == 0 else p.p_IM + ib
        M, I, srcM, srcI, slotI = [NINF] * n, [NINF] * n, [_BEGIN] * n, [0] * n, [0] * n
        for j, v in enumerate(nodes):
            b, r = NINF, _BEGIN + 1
            for u, t in par[v]:
                q = pslot.get(u)
                if q is None:
                    continue
                b, r = _take(b, r, t + (p.p_MM + pM[q]), (q << 2) | 0)
                b, r = _take(b, r, t + (p.p_IM + pI[q]), (q << 2) | 1)
                b, r = _take(b, r, t + (p.p_DM + pD[q]), (q << 2) | 2)
            b, r = _take(b, r, init[v] + beg_m, _BEGIN)
            M[j], srcM[j] = (p.p_match if emis[v] == x else p.p_mismatch) + b, r
            q = pslot.get(v)
            if q is not None:
                b, r = NINF, 4
                b, r = _take(b, r, p.p_MI + pM[q], 0)
                b, r = _take(b, r, p.p_II + pI[q], 1)
                b, r = _take(b, r, p.p_DI + pD[q], 2)
                I[j], srcI[j], slotI[j] = p.p_random + b, r, q
        ib = p.p_random + (p.p_MI if pos == 0 else p.p_II + ib)
        beg_d = p.p_ID + ib
        inlist = [[(slot[u], t) for u, t in par[v] if u in slot] for v in nodes]
        lv, srcD0 = [NINF] * n, [_BEGIN] * n
        for j, v in enumerate(nodes):
            b, r = NINF, _BEGIN + 1
            for q, t in inlist[j]:
                b, r = _take(b, r, t + (p.p_MD + M[q]), (q << 1) | 0)
                b, r = _take(b, r, t + (p.p_ID + I[q]), (q << 1) | 1)
            b, r = _take(b, r, init[v] + beg_d, _BEGIN)
            lv[j], srcD0[j] = b, r
        Dv, lvlD, parD = list(lv), [0] * n, [None]
        for t_ in range(1, G + 1):
            nx, pr = [NINF] * n, [0] * n
            for j in range(n):
                b, r = NINF, _BEGIN
                for q, t in inlist[j]:
                    b, r = _take(b, r, t + (p.p_DD + lv[q]), q)
                nx[j], pr[j] = b, r
                if b > Dv[j]:
                    Dv[j], lvlD[j] = b, t_
            parD.append(pr)
            lv = nx
        back.append((srcM, srcI, slotI, lvlD, srcD0, parD))
        pslot, pM, pI, pD = slot, M, I, Dv
    b, r = NINF, _BEGIN
    for j in range(len(pM)):
        b, r = _take(b, r, pM[j], (j << 2) | 0)
        b, r = _take(b, r, pI[j], (j << 2) | 1)
        b, r = _take(b, r, pD[j], (j << 2) | 2)
    best = p.p_end + b
    if not best > NINF:
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
    return best, rows


class IllegalPath(Exception):
    pass


def score_path(arrays, read, lists, rows):
    """Walks a path given in the out_path encoding from base 0 -> (ln P, n_terms, counts[4]); raises IllegalPath if it
    is no path of the model over these lists."""
    p = arrays.param
    G = int(p.n_max_gaps)
    emis, init = arrays.emission.tolist(), arrays.init_logp.tolist()
    edge = getattr(arrays, "_best_path_edges", None)
    if edge is None:
        edge = {}
        for u, v, t in zip(arrays.edge_src.tolist(), arrays.edge_dst.tolist(), arrays.trans_logp.tolist()):
            edge[(u, v)] = max(t, edge.get((u, v), NINF))  # parallel edges: a path takes the heavier
        arrays._best_path_edges = edge
    rows = np.asarray(rows)
    if rows.shape[0] != len(read):
        raise IllegalPath(f"{rows.shape[0]} rows for {len(read)} bases")
    terms, counts = [], [0, 0, 0, 0]
    to_m = {"M": p.p_MM, "I": p.p_IM, "D": p.p_DM, "IB": p.p_IM, "B": p.p_MM}
    to_i = {"M": p.p_MI, "I": p.p_II, "D": p.p_DI, "IB": p.p_II, "B": p.p_MI}
    to_d = {"M": p.p_MD, "I": p.p_ID, "D": p.p_DD, "IB": p.p_ID}
    kind, node = "B", None  # the state the path stands on
    for pos, x in enumerate(read):
        row, nodes = rows[pos].tolist(), lists[pos]
        used = [c for c in row if c != NONE]
        if row[:len(used)] != used:
            raise IllegalPath(f"base {pos}: the row does not end in padding: {row}")
        if not used:
            raise IllegalPath(f"base {pos}: empty row")
        if len(used) - 1 > G + 1:
            raise IllegalPath(f"base {pos}: {len(used) - 1} Dels in a row, n_max_gaps + 1 = {G + 1}")
        c = used[0]
        if c == INS_BEGIN:
            if kind not in ("B", "IB"):
                raise IllegalPath(f"base {pos}: InsBegin after a node state")
            terms += [to_i[kind], p.p_random]
            kind, node = "IB", None
            counts[2] += 1
        else:
            s, k = c >> 2, c & 3
            if k > 1:
                raise IllegalPath(f"base {pos}: entry 0 is no emitting state: {c:#x}")
            if s >= len(nodes):
                raise IllegalPath(f"base {pos}: slot {s} outside its list of {len(nodes)}")
            v = int(nodes[s])
            if k == 0:
                if kind in ("B", "IB"):
                    terms += [init[v], to_m[kind]]
                else:
                    if (node, v) not in edge:
                        raise IllegalPath(f"base {pos}: Match on {v} with no edge from {node}")
                    terms += [edge[(node, v)], to_m[kind]]
                terms.append(p.p_match if emis[v] == x else p.p_mismatch)
                counts[0 if emis[v] == x else 1] += 1
                kind, node = "M", v
            else:
                if kind in ("B", "IB") or node != v:
                    raise IllegalPath(f"base {pos}: Ins on {v} after {kind} {node}")
                terms += [to_i[kind], p.p_random]
                counts[2] += 1
                kind, node = "I", v
        for c in used[1:]:
            s, k = c >> 2, c & 3
            if c == INS_BEGIN or k != 2:
                raise IllegalPath(f"base {pos}: {c:#x} behind the emitting state is no Del")
            if s >= len(nodes):
                raise IllegalPath(f"base {pos}: Del slot {s} outside its list of {len(nodes)}")
            w = int(nodes[s])
            if kind == "IB":
                terms += [init[w], to_d[kind]]
            else:
                # (the source is the state before it in this row: a state of the same list by construction)
                if (node, w) not in edge:
                    raise IllegalPath(f"base {pos}: Del on {w} with no edge from {node}")
                terms += [edge[(node, w)], to_d[kind]]
            counts[3] += 1
            kind, node = "D", w
    if kind in ("B", "IB"):
        raise IllegalPath("the path never leaves Begin / InsBegin: it does not reach End")
    terms.append(p.p_end)
    return float(sum(terms)), len(terms), counts


def check_read(arrays, read, lists, logp, rows, counts):
    """what every parity test asks of one read's outputs -> (ref value, n_terms)"""
    want, _ = best_path_ref(arrays, read, lists)
    rows = np.asarray(rows)
    if want == NINF:
        assert logp == NINF and np.all(rows == NONE) and list(counts) == [0, 0, 0, 0], (logp, want)
        return want, 0
    got, n_terms, cnt = score_path(arrays, read, lists, rows)
    b = bar(n_terms, want)
    assert abs(logp - want) <= b, (logp, want, b)
    assert abs(got - logp) <= b, (got, logp, b)
    assert cnt == list(counts), (cnt, list(counts))
    return want, n_terms


# ---------------------------------------------------------------- the cases of the GPU tests (and of the CPU test)
WIDTHS = (64, 65, 128, 129, 400)
FUZZ_SEED, FUZZ_CASES = 20261020, (22, 23, 27, 37, 40, 48)


def linear(p):
    return D.mock_linear().to_phmm(D.PHMMParams.uniform(p))


def full_lists(arrays, read):
    return [list(range(arrays.n_nodes))] * len(read)


@functools.lru_cache(maxsize=None)
def fuzz_cases():
    """six cases of fuzz_cases.make_case, case c drawn from the stream seeded (FUZZ_SEED, c): the first six numbers whose
    reads keep the Python reference near 2e5 (entry, level) steps over all six (bases x 12 entries x levels as the
    estimate, at most 2e5 / 6 each; every read of a case stays).  n_max_gaps 0, 1, 4 and 6 are among them."""
    out = [make_case(np.random.default_rng([FUZZ_SEED, case]), case) for case in FUZZ_CASES]
    for c in out:
        assert sum(len(r) for r in c["reads"]) * 12 * (c["param"].n_max_gaps + 1) <= 2e5 / 6, c["tag"]
    return out


def two_deletions():
    """the DBG case and one read that carries two adjacent deletions: 92 bases of its first haplotype, bases 47 and 48
    out (there a path with one Del per base is 5.8 nats worse than the one with two Dels behind base 46)"""
    b = base_case("dbg")
    hap = bytes(D.random_genome(600, 3))  # (helpers.small_dbg_model(600, ., ., seed=3): the haplotype the DBG is built on)
    return b["arrays"], hap[100:147] + hap[149:192]


def pad_lists(po, nd, reads, n_nodes, width, seed=5):
    """the list of every read at two of every three positions padded with distinct other nodes, in shuffled order, to
    `width`; every third position keeps its own short list -> (pos_off, nodes)   (tests/test_gpu_edges_wide.py)"""
    rng = np.random.default_rng(seed)
    out_off, out = [0], []
    g = 0
    for r in reads:
        for i in range(len(r)):
            own = nd[int(po[g]):int(po[g + 1])]
            if i % 3 != 2 and own.size < width:
                others = np.setdiff1d(np.arange(n_nodes, dtype=np.uint32), own)
                lst = np.concatenate([own, rng.choice(others, size=width - own.size, replace=False).astype(np.uint32)])
                rng.shuffle(lst)
            else:
                lst = own
            out.append(lst)
            out_off.append(out_off[-1] + lst.size)
            g += 1
    return np.array(out_off, np.uint64), np.concatenate(out).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def repeat_case():
    """a short-unit repeat (100 bp x 10) at k = 24: 466 nodes, so that a list can be padded to 400 and to 401 distinct
    nodes, and lists of at most 27 nodes of its own"""
    arrays, reads, sg, _ = dataset("u100", 24, max_reads=4)
    return arrays, reads


def width_reads(width):
    """a few reads of at most 200 bases, fewer and shorter at the widest lists (two thirds of the positions are padded:
    bases x width x 2/3 x 5 levels stays near 2e5)"""
    arrays, reads = repeat_case()
    n, length = (3, 150) if width <= 65 else (2, 150) if width <= 129 else (2, 75)
    return arrays, [r[40 * j: 40 * j + length - 7 * j] for j, r in enumerate(reads[:n])]


@functools.lru_cache(maxsize=None)
def long_read():
    """one read of 3 000 bases on small_dbg_model"""
    arrays, _ = small_dbg_model(4000, 16, 0.01, seed=5, min_copy_num=1)
    for seed in range(1, 50):
        r = D.sample_reads(arrays, 10 ** 9, 3100, seed=seed, max_reads=1)[0]
        if len(r) >= 3000:
            return arrays, r[:3000]
    raise AssertionError("no read of 3000 bases")
