"""Reads drawn from the model in plain Python (test infrastructure, imported like sample_paths_ref.py): the restatement
phmm_sample_reads is held to -- the walk, the random stream and the draw rule exactly as include/phmm_amd_generate.h
writes them -- the exact law of short walks on a tiny model, the fixtures the CPU and the GPU tests share, and truth(),
which turns a walk's history into the lists and path rows of include/phmm_amd_path.h.

Every decision returns its margin as sample_paths_ref.draw does: the distance of u * c_last to the nearest inner boundary
of the running sums, divided by c_last.  The device's exp and Python's may differ in the last bits, so the two sides can
be compared word for word only where no decision lies that close to a boundary; the CPU test asserts it of every fixture
(a condition on the inputs, not a tolerance on the result)."""
import bisect
import functools
import itertools
import math

import numpy as np

import best_path_ref as B
from best_path_ref import INS_BEGIN, NINF, NONE, linear, score_path  # noqa: F401
from graph_cases import base_case
from sample_paths_ref import GOLD, MASK64, chi_bar, draw, mix, uniform  # noqa: F401

import dbgphmm_amd as D

STATE_COUNT, ENDABLE, EMIT_COUNT = 0, 1, 2
END = 0xFFFFFFFC
ENDED, DEAD_END, STATE_CAP, HISTORY_TRUNCATED = 1, 2, 4, 8
MIN_MARGIN = 1e-9
ACGT = b"ACGT"
M, I, DEL, MB, IB = 0, 1, 2, 3, 4  # the states of a walk; M, I, DEL are the kinds of a history word


def stream(seed, i):
    """x0 of walk i"""
    return mix((seed & MASK64) ^ mix((i + GOLD) & MASK64))


def state_cap(length):
    return 8 * length + 64


# ---------------------------------------------------------------- what a walk reads of the model
class Tables:
    __slots__ = ("out", "emis", "init", "init_c", "init_w_last", "param")


def tables(arrays):
    """cached on the arrays: out-edges per node in ascending edge index, and the running sums of the init pick (sequential
    double adds in node order)"""
    t = getattr(arrays, "_sample_reads_tables", None)
    if t is not None and t.param is arrays.param:
        return t
    t = Tables()
    t.param = arrays.param
    t.out = [[] for _ in range(arrays.n_nodes)]
    for u, v, x in zip(arrays.edge_src.tolist(), arrays.edge_dst.tolist(), arrays.trans_logp.tolist()):
        t.out[u].append((v, x))
    t.emis = arrays.emission.tolist()
    t.init = arrays.init_logp.tolist()
    t.init_c, t.init_w_last = running_sums(t.init)
    arrays._sample_reads_tables = t
    return t


def running_sums(terms):
    """-> (c[], index of the last candidate with w > 0); c is all zeros when no term is finite"""
    mx = max(terms) if terms else NINF
    if mx == NINF:
        return [0.0] * len(terms), 0
    w = [math.exp(x - mx) if x > NINF else 0.0 for x in terms]
    return list(itertools.accumulate(w)), max(k for k, x in enumerate(w) if x > 0.0)


def draw_sums(c, last, u):
    """the draw rule over prepared running sums, by bisection: the smallest i with u * c_last < c_i, else `last`
    -> (choice, margin)"""
    run = c[-1]
    thr = u * run
    k = bisect.bisect_right(c, thr)
    margin = math.inf
    for j in (k - 1, k):
        if 0 <= j < len(c) and 0.0 < c[j] < run:
            margin = min(margin, abs(thr - c[j]) / run)
    return (k if k < len(c) else last), margin


# ---------------------------------------------------------------- the walk
def walk(arrays, seed, i, length, kind, start_nodes=None, log=None):
    """walk i -> (bases, history words, flags without the truncation bit, smallest margin); log, if a list, receives
    (what, choice, margin) per decision"""
    p, t = arrays.param, tables(arrays)
    x0 = stream(seed, i)
    st = {"d": 0, "margin": math.inf}
    bases, hist = bytearray(), []
    pe = p.p_end if kind == ENDABLE else NINF
    nxt = {M: (p.p_MM, p.p_MI, p.p_MD, pe), I: (p.p_IM, p.p_II, p.p_ID, pe), DEL: (p.p_DM, p.p_DI, p.p_DD, pe),
           MB: (p.p_MI, p.p_MM, p.p_MD), IB: (p.p_II, p.p_IM, p.p_ID)}

    def decide(terms, what):
        """None (and no draw) when no term is finite"""
        if not any(x > NINF for x in terms):
            return None
        st["d"] += 1
        c, mg = draw(list(terms), uniform(x0, st["d"]))
        st["margin"] = min(st["margin"], mg)
        if log is not None:
            log.append((what, c, mg))
        return c

    def decide_sums(c, last, what):
        if not c or not c[-1] > 0.0:
            return None
        st["d"] += 1
        k, mg = draw_sums(c, last, uniform(x0, st["d"]))
        st["margin"] = min(st["margin"], mg)
        if log is not None:
            log.append((what, k, mg))
        return k

    def emit(state, node):
        if state == M:
            e = t.emis[node]
            terms = [p.p_match if b == e else p.p_mismatch for b in ACGT]
        else:
            terms = [p.p_random] * 4
        c = decide(terms, "emission")
        if c is None:
            return False
        bases.append(ACGT[c])
        return True

    def enter(state, node):
        hist.append((node << 2) | state if state <= DEL else INS_BEGIN if state == IB else END)

    flags, n_state = 0, 0
    state, node = MB, None
    alive = True
    if start_nodes is not None and len(start_nodes):
        c, last = running_sums([t.init[v] for v in start_nodes])
        node = int(start_nodes[decide_sums(c, last, "start")])
        state = M
        enter(M, node)
        if not emit(M, node):
            flags |= DEAD_END
            enter(END, None)
            n_state += 1
            alive = False
    while alive:
        ns = nn = None
        if state <= DEL:
            k = decide([x for _, x in t.out[node]], "child")
            if k is not None:
                child = t.out[node][k][0]
                c = decide(nxt[state], "state")
                if c is not None:
                    ns = (M, I, DEL, END)[c]
                    nn = node if c == 1 else child
        elif any(x > NINF for x in nxt[state]):
            v = decide_sums(t.init_c, t.init_w_last, "init")
            if v is not None:
                c = decide(nxt[state], "state")
                ns, nn = (IB, M, DEL)[c], v
        if ns is None:
            flags |= DEAD_END
            enter(END, None)
            n_state += 1
            break
        enter(ns, nn)
        n_state += 1
        if ns == END:
            flags |= ENDED
            break
        if ns in (M, I, IB) and not emit(ns, nn):
            flags |= DEAD_END
            enter(END, None)
            n_state += 1
            break
        state, node = ns, nn
        if (len(bases) >= length) if kind == EMIT_COUNT else (n_state >= length):
            break
        if n_state >= state_cap(length):
            flags |= STATE_CAP
            break
    return bytes(bases), hist, flags, st["margin"]


def usage_of(histories, n_nodes):
    """out_node_usage recounted from untruncated histories: Match, Ins and Del states per node"""
    use = np.zeros(n_nodes, dtype=np.uint32)
    for h in histories:
        for wd in h:
            if wd not in (INS_BEGIN, END, NONE):
                use[wd >> 2] += 1
    return use


def first_difference(arrays, seed, i, length, kind, start_nodes, history):
    """where walk i departs from `history` -> text with the margins of the decisions around that state"""
    log = []
    _, ref, _, _ = walk(arrays, seed, i, length, kind, start_nodes, log)
    got = [int(x) for x in history if x != NONE]
    k = next((j for j, (a, b) in enumerate(zip(got, ref)) if a != b), min(len(got), len(ref)))
    return (f"walk {i}: history word {k} is {got[k:k + 1]} for {ref[k:k + 1]} ({len(got)} words for {len(ref)}); the decisions: "
            + ", ".join(f"{w} -> {c} ({m:.2e})" for w, c, m in log[:3 * k + 6][-9:]))


# ---------------------------------------------------------------- the exact law of short walks
def chi_case():
    """4 nodes A, C, G, T: a branch 0 -> {1, 2}, a parallel edge 0 -> 1, a self-loop on 1, and 3 -> 0 back; STATE_COUNT
    at length 3"""
    prm = D.PHMMParams.new(0.1, 0.08, 0.2, 0.01, 40, 16)
    ln = lambda xs: np.log(np.array(xs, dtype=np.float64))
    src, dst, tr = [0, 0, 0, 1, 1, 2, 3], [1, 2, 1, 1, 3, 3, 0], [0.5, 0.3, 0.2, 0.4, 0.6, 1.0, 0.9]
    arrays = D.PHMMArrays(prm, np.frombuffer(b"ACGT", dtype=np.uint8).copy(), ln([0.5, 0.2, 0.2, 0.1]),
                          np.array(src, dtype=np.uint32), np.array(dst, dtype=np.uint32), ln(tr))
    return arrays, 3, STATE_COUNT


CHI_WALKS, CHI_SEED = 40000, 5


def _normalised(terms):
    mx = max(terms) if terms else NINF
    if mx == NINF:
        return None
    w = [math.exp(x - mx) if x > NINF else 0.0 for x in terms]
    s = sum(w)
    return [x / s for x in w]


def exact_law(arrays, length, kind=STATE_COUNT):
    """every walk of a tiny model from MatchBegin, with the normalised probability of each decision
    -> {(history tuple, bases): probability}; STATE_COUNT and ENDABLE only"""
    assert kind in (STATE_COUNT, ENDABLE)
    p, t = arrays.param, tables(arrays)
    pe = p.p_end if kind == ENDABLE else NINF
    nxt = {M: (p.p_MM, p.p_MI, p.p_MD, pe), I: (p.p_IM, p.p_II, p.p_ID, pe), DEL: (p.p_DM, p.p_DI, p.p_DD, pe),
           MB: (p.p_MI, p.p_MM, p.p_MD), IB: (p.p_II, p.p_IM, p.p_ID)}
    law = {}

    def word(state, node):
        return (node << 2) | state if state <= DEL else INS_BEGIN if state == IB else END

    def done(hist, bases, pr):
        key = (hist, bases)
        law[key] = law.get(key, 0.0) + pr

    def emissions(state, node):
        if state in (DEL, END):
            return [(b"", 1.0)]
        terms = [p.p_match if b == t.emis[node] else p.p_mismatch for b in ACGT] if state == M else [p.p_random] * 4
        pr = _normalised(terms)
        return None if pr is None else [(bytes([b]), q) for b, q in zip(ACGT, pr) if q > 0.0]

    def step(state, node, hist, bases, n_state, pr):
        if state <= DEL:
            firsts = _normalised([x for _, x in t.out[node]])
            firsts = None if firsts is None else [(t.out[node][k][0], q) for k, q in enumerate(firsts) if q > 0.0]
        else:
            firsts = _normalised(t.init)
            firsts = None if firsts is None else [(v, q) for v, q in enumerate(firsts) if q > 0.0]
        seconds = _normalised(nxt[state])
        if firsts is None or seconds is None:
            return done(hist + (END,), bases, pr)
        for v, q1 in firsts:
            for c, q2 in enumerate(seconds):
                if q2 == 0.0:
                    continue
                if state <= DEL:
                    ns, nn = (M, I, DEL, END)[c], (node if c == 1 else v)
                else:
                    ns, nn = (IB, M, DEL)[c], v
                h2 = hist + (word(ns, nn),)
                if ns == END:
                    done(h2, bases, pr * q1 * q2)
                    continue
                em = emissions(ns, nn)
                if em is None:
                    done(h2 + (END,), bases, pr * q1 * q2)
                    continue
                for b, q3 in em:
                    if n_state + 1 >= length:
                        done(h2, bases + b, pr * q1 * q2 * q3)
                    else:
                        step(ns, nn, h2, bases + b, n_state + 1, pr * q1 * q2 * q3)

    step(MB, None, (), b"", 0, 1.0)
    return law


def chi_square(law, outcomes):
    """outcomes: [(history tuple, bases)] of N walks -> (chi-square, df).  Cells: every outcome of the law whose
    expectation N p is >= 5; all others, unseen ones included, in one cell."""
    n = len(outcomes)
    seen = {}
    for key in outcomes:
        seen[key] = seen.get(key, 0) + 1
    assert all(key in law for key in seen), "an outcome the exact law does not hold"
    chi, cells, big_n, big_e = 0.0, 0, 0, 0.0
    for key, pr in law.items():
        e = n * pr
        if e >= 5.0:
            c = seen.get(key, 0)
            chi += (c - e) ** 2 / e
            cells += 1
            big_n += c
            big_e += e
    rest_e = n - big_e
    if rest_e > 1e-9 * n:
        chi += ((n - big_n) - rest_e) ** 2 / rest_e
        cells += 1
    return chi, cells - 1


# ---------------------------------------------------------------- the truth of a walk as lists and path rows
def truth(arrays, history, bases):
    """-> (lists[L], rows[L, n_max_gaps + 2]) of the walk in the layout of include/phmm_amd_path.h, the list of a base
    holding the nodes of its row, or None when the walk is outside the forward model: Begin to Del before any base, a
    Del run longer than n_max_gaps, or no node state at all (the path never leaves Begin / InsBegin)."""
    G = int(arrays.param.n_max_gaps)
    per_base = []
    on_node = False
    for wd in history:
        wd = int(wd)
        if wd in (END, NONE):
            continue
        if wd != INS_BEGIN and (wd & 3) == DEL:
            if not per_base:
                return None
            per_base[-1].append(wd)
            if len(per_base[-1]) - 1 > G:
                return None
        else:
            per_base.append([wd])
        on_node = on_node or wd != INS_BEGIN
    if not on_node or len(per_base) != len(bases) or not per_base:
        return None
    lists, rows = [], np.full((len(per_base), G + 2), NONE, dtype=np.uint32)
    for g, row in enumerate(per_base):
        nodes = []
        for wd in row:
            if wd != INS_BEGIN and (wd >> 2) not in nodes:
                nodes.append(wd >> 2)
        for j, wd in enumerate(row):
            rows[g, j] = INS_BEGIN if wd == INS_BEGIN else (nodes.index(wd >> 2) << 2) | (wd & 3)
        lists.append(nodes)
    # a base of InsBegin with no Del behind it names no node: its list takes the first node of the next list that has one
    for g in range(len(lists) - 1, -1, -1):
        if not lists[g]:
            lists[g] = [lists[g + 1][0]] if g + 1 < len(lists) and lists[g + 1] else [0]
    return lists, rows


# ---------------------------------------------------------------- the fixtures compared word for word
@functools.lru_cache(maxsize=None)
def model(name):
    if name == "linear":
        return linear(0.01)
    return base_case(name)["arrays"]


def _starts(arrays, k):
    """k start nodes with finite init, not in ascending order, one of them twice"""
    ok = np.flatnonzero(np.isfinite(arrays.init_logp))
    pick = ok[(np.arange(k) * 7 + 3) % ok.size]
    return [int(v) for v in pick[::-1]] + [int(pick[0])]


# (kind, length, walks, custom start, first index): every kind with and without start nodes, lengths 1, 2, 63, 257,
# walk counts 1, 63, 64, 65, 130
SHAPES = ((STATE_COUNT, 63, 65, False, 0), (ENDABLE, 257, 63, True, 5), (EMIT_COUNT, 63, 64, False, 1 << 33),
          (EMIT_COUNT, 2, 130, True, 0), (STATE_COUNT, 1, 1, False, 9), (ENDABLE, 2, 130, False, 64),
          (STATE_COUNT, 257, 64, True, 3), (EMIT_COUNT, 1, 65, True, 0), (ENDABLE, 1, 63, False, 0))
MODELS = ("dbg", "zoo", "linear")
# one seed per model; a fixture that fails the margin condition gets another seed here (never another threshold)
SEEDS = {"dbg": 101, "zoo": 102, "linear": 103}


@functools.lru_cache(maxsize=None)
def fixtures():
    out = []
    for name in MODELS:
        arrays = model(name)
        for kind, length, n, custom, first in SHAPES:
            out.append(dict(tag=f"{name} kind {kind} length {length} x {n}" + (" from start nodes" if custom else ""),
                            arrays=arrays, kind=kind, length=length, n_walks=n, first_index=first, seed=SEEDS[name],
                            start_nodes=_starts(arrays, 5) if custom else None))
    return out


@functools.lru_cache(maxsize=None)
def fixture_walks(k):
    """-> [(bases, history, flags, margin)] of fixture k"""
    f = fixtures()[k]
    return [walk(f["arrays"], f["seed"], f["first_index"] + w, f["length"], f["kind"], f["start_nodes"])
            for w in range(f["n_walks"])]
