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
    """what every parity test asks of one read's outputs -> (ref value, n_terms).  The value and the rows are held to
    best_path_ref EXACTLY: the kernel and the reference perform the same double additions in the same association and
    a maximum does not round, and the tie rule of the header fixes which of several equal paths is returned.  Only the
    re-scored sum of score_path, which adds the terms in another order, keeps the bar."""
    want, ref_rows = best_path_ref(arrays, read, lists)
    rows = np.asarray(rows)
    if want == NINF:
        assert logp == NINF and np.all(rows == NONE) and list(counts) == [0, 0, 0, 0], (logp, want)
        return want, 0
    got, n_terms, cnt = score_path(arrays, read, lists, rows)
    b = bar(n_terms, want)
    assert abs(logp - want) <= b, (logp, want, b)
    assert abs(got - logp) <= b, (got, logp, b)
    assert cnt == list(counts), (cnt, list(counts))
    assert logp == want, (logp, want, logp - want)
    if not np.array_equal(rows, ref_rows):
        g = int(np.flatnonzero((rows != ref_rows).any(axis=1))[-1])  # the walk goes backwards: the last row departs first
        raise AssertionError(f"the path departs from the reference's at base {g}: {rows[g].tolist()} for {ref_rows[g].tolist()}")
    assert list(counts) == score_path(arrays, read, lists, ref_rows)[2], (list(counts), ref_rows)
    return want, n_terms


def features(rows):
    """what a path in the out_path encoding shows -> {name: count}: every transition 'X>Y' between consecutive states
    (B, IB, M, I, D), the end 'end X', and 'full Del row' per row that holds n_max_gaps + 1 Dels.  Empty for a read
    without a path."""
    rows = np.asarray(rows)
    out = {}
    if rows.size == 0 or rows[0, 0] == NONE:
        return out
    kind = "B"
    for row in rows.tolist():
        used = [c for c in row if c != NONE]
        for c in used:
            k = "IB" if c == INS_BEGIN else "MID"[c & 3]
            out[f"{kind}>{k}"] = out.get(f"{kind}>{k}", 0) + 1
            kind = k
        if len(used) == len(row):
            out["full Del row"] = out.get("full Del row", 0) + 1
    out[f"end {kind}"] = 1
    return out


FEATURES = ("B>M", "B>IB", "IB>IB", "IB>M", "IB>D", "M>M", "M>I", "M>D", "I>M", "I>I", "I>D", "D>M", "D>I", "D>D",
            "end M", "end I", "end D", "full Del row")


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


# ---------------------------------------------------------------- ties, odd lists and -inf parameters (CPU and GPU tests)
# Integer logs: every sum is exact, so equal path values are equal doubles and the tie rule decides everywhere.  Match
# dominates (0 for a matching base, -4 for another); opening a gap costs 3 and leaving it 1, so that one mismatch, one
# deleted node (p_MD + p_DM) and an inserted base (p_MI + p_random + p_IM = -5) stay comparable and chains of two or
# three (p_DD = p_II = -1) are cheaper than mismatching the rest of the read.
INT_LOGS = dict(p_mismatch=-4, p_match=0, p_random=-1, p_gap_open=-3, p_gap_ext=-1, p_end=-1,
                p_MM=0, p_IM=-1, p_DM=-1, p_MI=-3, p_II=-1, p_DI=-3, p_MD=-3, p_ID=-3, p_DD=-1)
INF_PARAMS = ("p_MM", "p_IM", "p_DM", "p_MI", "p_II", "p_DI", "p_MD", "p_ID", "p_DD", "p_mismatch")
N_ISOLATED = 400
CASE_SEED = 20261021


def int_params(gaps, **over):
    kw = {k: float(v) for k, v in {**INT_LOGS, **over}.items()}
    return D.PHMMParams(n_active_nodes=40, active_node_max_ratio=30.0, n_warmup=16, warmup_threshold=200,
                        n_max_gaps=gaps, **kw)


def ordinary_params(gaps, **over):
    return D.PHMMParams.new(0.07, 0.11, 0.23, 0.01, 40, 16).with_(n_max_gaps=gaps, **over)


def int_logs(x):
    """the logs rounded to integers (-inf stays, no -0.0)"""
    x = np.asarray(x, dtype=np.float64)
    return np.where(np.isfinite(x), np.round(np.where(np.isfinite(x), x, 0.0)) + 0.0, NINF)


def with_isolated(arrays, k=N_ISOLATED):
    """the model with k more nodes behind its own: no edges and init = -inf, so every state on them is -inf on every
    list ("-inf is never chosen": entries that name them change no value and no choice)"""
    emit = None if arrays.is_emittable is None else np.concatenate([arrays.is_emittable, np.ones(k, arrays.is_emittable.dtype)])
    return D.PHMMArrays(arrays.param, np.concatenate([arrays.emission, np.full(k, ord("A"), np.uint8)]),
                        np.concatenate([arrays.init_logp, np.full(k, NINF)]), arrays.edge_src, arrays.edge_dst,
                        arrays.trans_logp, emit)


def pad_unreachable(lists, first_pad, width, front):
    """every list of one read padded to `width` with the isolated nodes first_pad, first_pad + 1, .., behind its own
    entries or in front of them (a list that is as long already stays)"""
    out = []
    for lst in lists:
        pad = list(range(first_pad, first_pad + max(0, width - len(lst))))
        out.append(pad + list(lst) if front else list(lst) + pad)
    return out


def shift_slots(rows, lists, width):
    """rows over lists as rows over pad_unreachable(lists, ., width, front=True): every slot moves by the pad count"""
    rows = np.array(rows, dtype=np.uint32)
    for g, lst in enumerate(lists):
        node = (rows[g] != NONE) & (rows[g] != INS_BEGIN)
        rows[g, node] += np.uint32(max(0, width - len(lst)) << 2)
    return rows


def csr(per_read_lists):
    """the lists of several reads, one after the other -> (pos_off, nodes)"""
    flat = [lst for lists in per_read_lists for lst in lists]
    off = np.zeros(len(flat) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in flat])
    return off, np.array([v for x in flat for v in x], dtype=np.uint32)


def bubble_case():
    """0 -> {1, 2} -> 3 -> {4, 5} -> 6 with equal branches that emit the same base: two ties, each decided by the slot
    order of the list -> (arrays, read, {name: (list order, the nodes of the path)})"""
    ln = math.log
    arrays = D.PHMMArrays(D.PHMMParams.uniform(0.01).with_(n_max_gaps=2), np.frombuffer(b"ACCGTTA", dtype=np.uint8).copy(),
                          np.full(7, ln(1.0 / 7.0)), np.array([0, 0, 1, 2, 3, 3, 4, 5], np.uint32),
                          np.array([1, 2, 3, 3, 4, 5, 6, 6], np.uint32),
                          np.array([ln(0.5), ln(0.5), 0.0, 0.0, ln(0.5), ln(0.5), 0.0, 0.0]))
    orders = {"ascending": ([0, 1, 2, 3, 4, 5, 6], [0, 1, 3, 4, 6]), "reversed": ([6, 5, 4, 3, 2, 1, 0], [0, 2, 3, 5, 6]),
              "2 before 1": ([0, 2, 1, 3, 4, 5, 6], [0, 2, 3, 4, 6]), "5 before 4": ([3, 5, 0, 1, 6, 4, 2], [0, 1, 3, 5, 6])}
    return arrays, b"ACGTA", orders


def _edit(rng, r, j):
    """a read of at most 40 bases with two adjacent deletions, two inserted bases, or a substitution and a deletion (a
    read of fewer than 20 bases stays as it is)"""
    r = bytearray(r[:38])
    if len(r) < 20:
        return bytes(r)
    a = int(rng.integers(6, len(r) - 12))
    if j % 3 == 0:
        del r[a:a + 2]
    elif j % 3 == 1:
        r[a:a] = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=2))
    else:
        r[a] = b"ACGT"[(b"ACGT".index(r[a]) + 1) % 4]
        del r[a + 9:a + 10]
    return bytes(r)


def _oracle_lists(arrays, reads):
    from oracle import oracle as O
    O.build()
    (po, nd, lp), _ = O.Model(arrays).generate_mappings(reads, None, True, n_threads=8)
    return po, nd, lp


@functools.lru_cache(maxsize=None)
def int_case(graph):
    """base_case(graph) in integer logs -> dict(arrays, reads, lists[read][pos], n_real): the model's logs rounded,
    int_params, N_ISOLATED isolated nodes behind the n_real real ones; 12 edited reads of at most 40 bases; per position a
    shuffled list of 20 to 60 real nodes: the first 12 at most of the oracle's own list for that position on the ordinary
    model (the neighbourhood of the path) and random others.
    Where the ties come from.  dbg: the two branches of a SNP bubble emit the same bases behind the SNP and have equal
    rounded weights, so a read that starts inside one is placed by slot order.  zoo: the seven arms of the hub get the
    bases of arm 0 here (their rounded weights are equal already), and a read that crosses the hub is cut so that it
    keeps the crossing: on any arm but 0 it mismatches all seven alike."""
    b = base_case(graph)
    a = b["arrays"]
    rng = np.random.default_rng([CASE_SEED, ("zoo", "dbg").index(graph)])
    emission = a.emission.copy()
    full = b["reads"]
    if graph == "zoo":
        for arm in range(1, 7):
            emission[150 + 4 * arm:154 + 4 * arm] = emission[150:154]
        po, nd, lp = _oracle_lists(a, full)
        cut, g = [], 0
        for r in full:  # the window of 38 bases starts 12 bases before the read's first base on node 60, if it has one
            top = [int(nd[int(po[g + i]):int(po[g + i + 1])][np.argmax(lp[int(po[g + i]):int(po[g + i + 1])])]) for i in range(len(r))]
            s = max(0, top.index(60) - 12) if 60 in top else 0
            cut.append(r[s:] if len(r) - s >= 30 else r)
            g += len(r)
        full = cut
    reads = [_edit(rng, r, j) for j, r in enumerate(full)]
    po, nd, lp = _oracle_lists(a, reads)
    lists, g = [], 0
    for r in reads:
        per = []
        for _ in r:
            e0, e1 = int(po[g]), int(po[g + 1])
            hood = nd[e0:e1][np.argsort(-lp[e0:e1], kind="stable")][:12].astype(np.int64)
            n = int(rng.integers(20, 61))
            others = rng.choice(np.setdiff1d(np.arange(a.n_nodes), hood), size=n - hood.size, replace=False)
            lst = np.concatenate([hood, others])
            rng.shuffle(lst)
            per.append(lst.tolist())
            g += 1
        lists.append(per)
    ia = D.PHMMArrays(int_params(2 if graph == "zoo" else 3), emission, int_logs(a.init_logp), a.edge_src, a.edge_dst,
                      int_logs(a.trans_logp), a.is_emittable)
    return dict(arrays=with_isolated(ia), reads=reads, lists=lists, n_real=a.n_nodes)


def reversed_lists(lists):
    return [[lst[::-1] for lst in per] for per in lists]


# The odd graph: 9 nodes, a chain 0 -> 1 -> .. -> 8 with a branch 0 -> 2, a skip 2 -> 4, a self-loop 5 -> 5, a back edge
# 6 -> 3 and the edge 1 -> 2 twice with different weights.
_ODD_BASES = b"ACGTTACGA"
_ODD_EDGES = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (6, 7), (7, 8), (0, 2), (2, 4), (5, 5), (6, 3), (1, 2)]
_ODD_TRANS = [0.6, 0.5, 0.55, 0.9, 0.8, 0.45, 0.7, 0.95, 0.3, 0.35, 0.4, 0.2, 0.25]
_ODD_INIT = [0.3, 0.1, 0.12, 0.08, 0.1, 0.09, 0.07, 0.06, 0.05]


def odd_arrays(flavour, gaps, init_only=None, **over):
    """the odd graph with ordinary (unnormalised, all different) or integer logs; init_only: init is -inf on every other
    node; over: parameters to replace"""
    init, trans = np.log(_ODD_INIT), np.log(_ODD_TRANS)
    if flavour == "int":
        init, trans = int_logs(init), int_logs(2.0 * trans)
    if init_only is not None:
        init = np.where(np.arange(init.size) == init_only, init, NINF)
    p = (int_params if flavour == "int" else ordinary_params)(gaps, **over)
    e = np.array(_ODD_EDGES, dtype=np.uint32)
    return D.PHMMArrays(p, np.frombuffer(_ODD_BASES, dtype=np.uint8).copy(), init, e[:, 0].copy(), e[:, 1].copy(), trans)


def _odd_walk(rng, length, start=None):
    succ = {}
    for u, v in _ODD_EDGES:
        succ.setdefault(u, []).append(v)
    v = int(rng.integers(0, 6)) if start is None else start
    walk = [v]
    while len(walk) < length and v in succ:
        v = int(rng.choice(succ[v]))
        walk.append(v)
    return walk


def _odd_read(rng, length, noise=True, start=None):
    """a walk of `length` nodes, its bases with (noise) some nodes left out or a base put in or replaced, and per base a
    shuffled list of 3 to 9 nodes that holds the node the base came from most of the time -> (read, lists, walk)"""
    walk = _odd_walk(rng, length + 3 if noise else length, start)
    src = list(walk)
    if noise and len(src) > 3:
        what = int(rng.integers(0, 4))
        a = int(rng.integers(1, len(src) - 1))
        if what == 0:
            del src[a:a + int(rng.integers(1, 4))]
        elif what == 1:
            src[a:a] = [None] * int(rng.integers(1, 3))
        elif what == 2:
            src[a] = None
    src = src[:length]
    read, lists = bytearray(), []
    for v in src:
        read.append(_ODD_BASES[v] if v is not None else b"ACGT"[int(rng.integers(0, 4))])
        lst = rng.permutation(9)[:int(rng.integers(3, 10))].tolist()
        if v is not None and v not in lst and rng.random() < 0.8:
            lst[int(rng.integers(0, len(lst)))] = v
        lists.append(lst)
    return bytes(read), lists, walk


def _odd_list_kinds(rng):
    """the list oddities, each on fresh reads -> [(kind, read, lists, cause of -inf or None)]"""
    out = []
    for s in range(4):
        read, lists, _ = _odd_read(rng, int(rng.integers(4, 10)))
        for lst in lists:
            a = int(rng.integers(0, len(lst)))
            lst.insert(a, lst[a])
        out.append(("duplicates, adjacent", read, lists, None))
        read, lists, _ = _odd_read(rng, int(rng.integers(4, 10)))
        out.append(("duplicates, apart", read, [lst + [lst[0]] if len(lst) > 1 else lst for lst in lists], None))
        read, lists, _ = _odd_read(rng, int(rng.integers(3, 10)))
        out.append(("empty list at position 0", read, [[]] + lists[1:], None))
        read, lists, _ = _odd_read(rng, int(rng.integers(3, 10)))
        mid = len(read) // 2
        out.append(("empty list in the middle", read, lists[:mid] + [[]] + lists[mid + 1:], None))
        read, lists, _ = _odd_read(rng, int(rng.integers(3, 10)))
        out.append(("empty list at the last position", read, lists[:-1] + [[]], "empty last list"))
        read, lists, _ = _odd_read(rng, 1, noise=False)
        out.append(("one base", read, lists, None))
        read, lists, walk = _odd_read(rng, int(rng.integers(5, 10)), noise=False, start=5)  # (5 -> 5: the node can stay)
        lists = [lst if 5 in lst else lst + [5] for lst in lists]
        mid = len(read) // 2
        lists[mid] = [v for v in lists[mid] if v != 5]
        out.append(("a node leaves the list and comes back", read, lists, None))
        read, lists, _ = _odd_read(rng, int(rng.integers(4, 10)))
        out.append(("plain", read, lists, None))
    return out


def odd_arrays_free_dels(flavour, gaps):
    """the odd graph with p_MD = p_DD = 0 and weight 1 on 2 -> 3, 3 -> 4, 2 -> 4, 4 -> 5 and 7 -> 8: a Del behind a Match
    on 2, 3 or 7 has exactly the value of that Match (x + 0 is x), so that ties between a state and the Dels behind it,
    and between the Del levels of 4 behind a Match on 2 (2 -> 4 and 2 -> 3 -> 4), occur with any logs"""
    a = odd_arrays(flavour, gaps, p_MD=0.0, p_DD=0.0)
    for e in (2, 3, 4, 7, 9):
        a.trans_logp[e] = 0.0
    return a


def _shuffled_full(rng, n):
    return [rng.permutation(9).tolist() for _ in range(n)]


def _forms(rng, flavour):
    """Path forms that the list oddities seldom show, forced by -inf parameters on full lists in shuffled order
    -> [(tag, arrays, cases)].  With p_mismatch = -inf every Match must emit the read's base, so a base put in is an Ins
    or InsBegin and a node left out a Del; p_MI = -inf besides leaves only Dels.  Bases of the nodes 0..8: A C G T T A C G A
    (the chain 0 -> .. -> 8, 0 -> 2, 2 -> 4, 5 -> 5, 6 -> 3).  The comments name the walk a read is made from; what
    the best path is, the reference decides."""
    N = NINF
    out = []

    def cases(reads, copies, cause="-inf parameters"):
        return [(f"form {r.decode()}", r, _shuffled_full(rng, len(r)), cause) for r in reads for _ in range(copies)]
    # a base or two put in: in front of 1 2 3 4 5, between 3 and 4, between 6 and 7
    out.append(("forms, p_mismatch = -inf", odd_arrays(flavour, 2, p_mismatch=N), cases((b"CCGTTA", b"GTCCTAC", b"TACTAGA"), 3)))
    # nodes left out: 3 [4 5 6] 7 8, 3 4 [5 6] 7 8, 5 6 [3 4 5] 6 7 8, 2 3 [4 5 6] 7 8 or 2 4 [5 6] 7 8
    out.append(("forms, p_mismatch = p_MI = -inf", odd_arrays(flavour, 2, p_mismatch=N, p_MI=N),
                cases((b"TGA", b"TTGA", b"ACCGA", b"GTGA"), 2)))
    # one Del per row at most: 3 4 [5] 6 7 8, 2 4 5 6 [7] 8, and 3 [4 5 6] 7 8, which has no path then
    out.append(("forms, p_mismatch = p_MI = -inf, n_max_gaps = 0", odd_arrays(flavour, 0, p_mismatch=N, p_MI=N),
                cases((b"TTCGA", b"GTACA", b"TGA"), 2)))
    # 2 3 4, a base put in, 5 left out, 6 7 8: Ins then Del, or Del then Ins; and reads that have no Match and no way
    # from InsBegin to a Del
    for name in ("p_ID", "p_DI"):
        c = cases((b"GTTGCGA", b"TTGCGA", b"CGTTGCGA"), 2)
        c += [("no Match emits the base", b"T", [[0, 1]], "-inf parameters"), ("no Match emits the base", b"GG", [[0, 1], [3]], "-inf parameters")]
        out.append((f"forms, p_mismatch = {name} = -inf", odd_arrays(flavour, 2, **{"p_mismatch": N, name: N}), c))
    # init on node 2 alone, the read starts with a base that 2 does not emit and goes on from 3: InsBegin, Del on 2
    out.append(("forms, p_mismatch = -inf, init on node 2", odd_arrays(flavour, 2, init_only=2, p_mismatch=N),
                cases((b"ATTA", b"CTT", b"TTTAC", b"AATT"), 1)))
    # free Dels: the read ends on 2, 3 or 7 with the child in front of it in the list -> the end state is the Del (lower
    # rank), and the Del on 4 behind a Match on 2 is held at level 0 and, through 3, at level 1: the lower level
    for gaps in (0, 2):
        c = []
        for r, last in ((b"CGT", [4, 3, 5]), (b"ACG", [8, 2, 7]), (b"GT", [5, 4, 3]), (b"CG", [7, 8]), (b"TTACG", [8, 0, 7, 1]),
                        (b"CG", [4, 2, 3]), (b"ACG", [4, 3, 2, 8])):
            c.append(("ties between a Match and the Dels behind it", r, _shuffled_full(rng, len(r) - 1) + [last], None))
        out.append((f"free Dels, n_max_gaps = {gaps}", odd_arrays_free_dels(flavour, gaps), c))
    return out


@functools.lru_cache(maxsize=None)
def odd_cases(flavour):
    """-> groups [dict(tag, arrays, reads, lists[read][pos], kinds[read], causes[read])], one model each: the list
    oddities at n_max_gaps 0, 1 and 2, each of INF_PARAMS at -inf in turn (random reads and a read of one base), init =
    -inf on all but one node with that node on the lists (reachable) and off them (an unreachable start), and the forced
    path forms of _forms.  causes[read] names why the read may have no path (None: it should have one)."""
    rng = np.random.default_rng([CASE_SEED, 7, ("ord", "int").index(flavour)])
    groups = []

    def group(tag, arrays, cases):
        groups.append(dict(tag=f"{flavour}: {tag}", arrays=arrays, reads=[c[1] for c in cases], lists=[c[2] for c in cases],
                           kinds=[c[0] for c in cases], causes=[c[3] for c in cases]))
    for gaps in (0, 1, 2):
        group(f"list oddities, n_max_gaps = {gaps}", odd_arrays(flavour, gaps), _odd_list_kinds(rng))
    for name in INF_PARAMS:
        cases = []
        for s in range(4):
            read, lists, _ = _odd_read(rng, int(rng.integers(3, 10)))
            cases.append((f"{name} = -inf", read, lists, "-inf parameters"))
        cases.append((f"{name} = -inf, one base", b"T", [[0, 3, 1]], "-inf parameters"))
        group(f"{name} = -inf", odd_arrays(flavour, 2, **{name: NINF}), cases)
    cases = []
    for s in range(6):
        # the only node with an init is 2; the read starts with a base of its own, then follows 3 -> 4 -> ..: InsBegin,
        # then Match on 2 or a Del on it in front of 3
        read, lists, _ = _odd_read(rng, int(rng.integers(3, 7)), noise=False, start=3)
        read = b"ACGT"[s % 4:s % 4 + 1] * (1 + s % 2) + read
        lists = [[] if s % 3 == 0 else [2, 7]] * (1 + s % 2) + [lst if 2 in lst else [2] + lst for lst in lists]
        cases.append(("init on one node, listed", read, lists, None))
    group("init on one node, listed", odd_arrays(flavour, 2, init_only=2), cases)
    cases = []
    for s in range(4):
        read, lists, _ = _odd_read(rng, int(rng.integers(2, 8)))
        cases.append(("init on one node, never listed", read, [[v for v in lst if v != 8] for lst in lists], "unreachable start"))
    group("init on one node, never listed", odd_arrays(flavour, 2, init_only=8), cases)
    for tag, arrays, cases in _forms(rng, flavour):
        group(tag, arrays, cases)
    return groups


@functools.lru_cache(maxsize=None)
def many_short_reads(n=320):
    """n reads of 1 to 12 bases on the odd graph (ordinary logs, n_max_gaps = 2) with lists of at most 8 nodes, some with
    a duplicate -> (arrays, reads, lists[read][pos])"""
    rng = np.random.default_rng([CASE_SEED, 11])
    reads, lists = [], []
    for j in range(n):
        read, ls, _ = _odd_read(rng, 1 + j % 12, noise=j % 12 > 2)
        ls = [lst[:7] for lst in ls]
        reads.append(read)
        lists.append([lst + [lst[0]] if j % 5 == 0 else lst for lst in ls])
    return odd_arrays("ord", 2), reads, lists
