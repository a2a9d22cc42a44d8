"""Time the greedy search of sample_posterior (multi_dbg/posterior.rs:314-417) on the phmm_likelihood handle with
the candidates stated in the sampler's own units -- compact edges, here the unitig groups of the graph -- two ways:

  side A  the node form: the caller expands every group change into (node, cn) pairs (what INTEGRATION.md section 3
          asked of it before groups: the loop over edges_in_full, here one vectorised numpy gather) and calls
          score_changes + move.  The expansion is inside A's clock: it is work the caller has to do.
  side B  the group form: score_group_changes + move_groups on the group lists as they are.

Both sides live in one library, so one process alternates them: per cell one warm-up search each, then `--reps` rounds
A, B, A, B ...; a search is `--iters` iterations from the graph's own copy numbers, each scoring C candidates and moving
to one of them (fixed seed: both sides walk the same sequence).  Only totals are asked for (out_logp = NULL), as the
sampler does.  Every iteration's totals and rescored counts, and the state after the last move (vector, per-read
values, total), are compared between the two sides: `max_abs_delta` must be 0.

Shapes:
  bubble  cfg3 (100 kb x 2, 1 % divergence, k = 40): bubble swaps, both arms as groups, +1 / -1 with a floor of 0
  long    the cfg3 genome at 0.1 % divergence: candidates moving 4 random groups of at least 200 nodes by +-1

    python tools/likelihood_groups_time.py [--cands 64,256,1024] [--shapes bubble,long] [--iters 20] [--reps 5]

Prints one JSON line per cell: ms per iteration of both sides (median, min, max), A's spread, A / B, the share of A's
time spent expanding, node and group changes per iteration, and whether B <= A + A's spread.  The split of a call into
its sections is a run of its own, because the trace synchronises the stream at every section: the same command under
PHMM_TRACE=1 with --reps 1 --iters 3 (the sections go to standard error, a '[side A]' / '[side B]' line in front of
each search).  profiles/likelihood_groups.txt holds both.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def csr(cands):
    off = np.zeros(len(cands) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(n) for n, _ in cands])
    ids = np.concatenate([np.asarray(n, np.uint32) for n, _ in cands] + [np.zeros(0, np.uint32)])
    cn = np.concatenate([np.asarray(v, np.uint32) for _, v in cands] + [np.zeros(0, np.uint32)])
    return off, ids, cn


def expand(goff, gnodes, off, grp, cn):
    """group CSR -> node CSR: (g, cn) becomes (v, cn) for every node v of g (one gather, no Python loop)"""
    sizes = (goff[1:] - goff[:-1])[grp]
    ends = np.cumsum(sizes)
    total = int(ends[-1]) if ends.size else 0
    starts = ends - sizes
    src = np.repeat(goff[:-1][grp] - starts, sizes) + np.arange(total)
    node_off = np.concatenate([[0], ends])[off.astype(np.int64)].astype(np.uint64)
    return node_off, gnodes[src], np.repeat(cn, sizes)


def bubble_groups(D, sg, occ, goff, gnodes, group_of):
    """bubbles whose two arms are whole groups -> [(groups of the hap-A arm, groups of the hap-B arm)]"""
    a, b = occ
    in_a, in_b = np.zeros(sg.base.size, bool), np.zeros(sg.base.size, bool)
    in_a[a] = True
    in_b[b] = True
    pos_b = {int(v): i for i, v in enumerate(b)}
    shared = np.flatnonzero(in_b[a])
    sizes = np.diff(goff)
    out = []
    for i in range(shared.size - 1):
        lo, hi = shared[i], shared[i + 1]
        if hi - lo < 3 or int(a[lo]) not in pos_b or int(a[hi]) not in pos_b:
            continue
        ib, jb = pos_b[int(a[lo])], pos_b[int(a[hi])]
        if jb <= ib:
            continue
        a_only = np.unique(a[lo + 1:hi][~in_b[a[lo + 1:hi]]])
        b_only = np.unique(b[ib + 1:jb][~in_a[b[ib + 1:jb]]])
        if not (a_only.size and b_only.size):
            continue
        ga, gb = np.unique(group_of[a_only]), np.unique(group_of[b_only])
        if sizes[ga].sum() == a_only.size and sizes[gb].sum() == b_only.size:
            out.append((ga, gb))
    return out


def candidates(shape, gvec, pool, Cn, it):
    """C candidates in group units -> [(groups, new cns)] (seeded by the iteration: the same for both sides)"""
    rng = np.random.default_rng(1000 + it)
    out = []
    for c in range(Cn):
        if shape == "bubble":
            ga, gb = pool[(it * 7 + c) % len(pool)]
            out.append((np.concatenate([ga, gb]),
                        np.concatenate([gvec[ga].astype(np.int64) + 1, np.maximum(gvec[gb].astype(np.int64) - 1, 0)])))
        else:
            gs = rng.choice(pool, size=4, replace=False)
            out.append((gs, np.maximum(gvec[gs].astype(np.int64) + rng.choice([-1, 1], size=4), 0)))
    return out


def build(shape):
    import bench  # (workload builders only)
    import dbgphmm_amd as D
    w = bench.WORKLOADS["cfg3"]
    hap = D.random_genome(w["genome"], seed=3)
    haps = [hap, D.diverge(hap, 0.01 if shape == "bubble" else 0.001, seed=4)]
    sg, occ = D.dbg_from_haplotypes(haps, w["k"], with_occurrences=True)
    param = D.PHMMParams.uniform(w["p"]).with_(n_warmup=w["k"])
    arrays = D.vectorised_to_phmm(sg, param, 1)
    reads = D.sample_reads(arrays, w["coverage"] * w["genome"] * 2, w["read_len"], seed=1000)
    model = D.PHMMModel(arrays)
    rc = D.ReadCollection(reads)
    mp, _ = model.generate_mappings(rc, None, True)
    goff, gnodes = D.unitig_groups(sg)
    goff = goff.astype(np.int64)
    sizes = np.diff(goff)
    group_of = np.empty(sg.base.size, np.int64)
    group_of[gnodes] = np.repeat(np.arange(sizes.size), sizes)
    base = sg.copy_num.astype(np.uint32)
    pool = bubble_groups(D, sg, occ, goff, gnodes, group_of) if shape == "bubble" else np.flatnonzero(sizes >= 200)
    info = dict(shape=shape, n_nodes=int(base.size), n_groups=int(sizes.size), median_group=float(np.median(sizes)),
                largest_group=int(sizes.max()), groups_of_200_or_more=int((sizes >= 200).sum()), reads=len(reads),
                pool=len(pool))
    return model, rc, mp, base, goff, gnodes, pool, info


def search(side, shape, model, rc, mp, base, goff, gnodes, pool, Cn, iters):
    """one search -> (ms per iteration, ms of it expanding, per-iteration outputs, final state, changes per iteration)"""
    from dbgphmm_amd import _ffi
    L = _ffi.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    lk = model.likelihood(rc, mp, base, 0)
    lk.set_groups(goff, gnodes)
    gvec = base[gnodes[goff[:-1]]].copy()
    pick = np.random.default_rng(7).integers(0, Cn, size=iters)
    tot, nres = np.empty(Cn), np.empty(Cn, np.uint64)
    ms = ms_expand = 0.0
    outs, n_node, n_group = [], 0, 0
    if os.environ.get("PHMM_TRACE"):
        print("[side %s] %s C=%d" % (side, shape, Cn), file=sys.stderr, flush=True)
    for it in range(iters):
        cands = candidates(shape, gvec, pool, Cn, it)
        off, grp, cn = csr(cands)
        mg, mv = np.asarray(cands[pick[it]][0], np.uint32), np.asarray(cands[pick[it]][1], np.uint32)
        moff = np.array([0, mg.size], np.uint64)
        n_group += grp.size + mg.size
        t0 = time.perf_counter()
        if side == "A":
            noff, node, ncn = expand(goff, gnodes, off, grp, cn)
            _, mnode, mcn = expand(goff, gnodes, moff, mg, mv)
            t1 = time.perf_counter()
            ms_expand += (t1 - t0) * 1e3
            _ffi.check(L.phmm_likelihood_score_changes(lk._h, Cn, p(noff), p(node), p(ncn), None, p(tot), p(nres)))
            mt = lk.move(mnode, mcn)
            n_node += node.size + mnode.size
        else:
            _ffi.check(L.phmm_likelihood_score_group_changes(lk._h, Cn, p(off), p(grp), p(cn), None, p(tot), p(nres)))
            mt = lk.move_groups(mg, mv)
        ms += (time.perf_counter() - t0) * 1e3
        gvec[mg] = mv
        outs.append((tot.copy(), nres.astype(np.float64), np.array(mt, dtype=np.float64)))
    cur_cn, cur_lp, cur_tot = lk.current()
    outs.append((cur_cn.astype(np.float64), cur_lp, np.array([cur_tot])))
    return ms / iters, ms_expand / iters, outs, n_node / iters, n_group / iters


def max_delta(oa, ob):
    d = 0.0
    for xa, xb in zip(oa, ob):
        for a, b in zip(xa, xb):
            with np.errstate(invalid="ignore"):
                e = np.where((a == b) | (np.isnan(a) & np.isnan(b)), 0.0, np.abs(a - b))
            d = max(d, float(np.max(e)) if e.size else 0.0)
            if np.any(np.isnan(e)):
                return float("inf")
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cands", default="64,256,1024")
    ap.add_argument("--shapes", default="bubble,long")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    for shape in args.shapes.split(","):
        model, rc, mp, base, goff, gnodes, pool, info = build(shape)
        print(json.dumps(info), flush=True)
        for Cn in (int(x) for x in args.cands.split(",")):
            run = lambda side: search(side, shape, model, rc, mp, base, goff, gnodes, pool, Cn, args.iters)  # noqa: E731
            if not os.environ.get("PHMM_TRACE"):
                run("A")
                run("B")  # warm-up: one search each
            ta, tb, te, delta = [], [], [], 0.0
            for _ in range(args.reps):
                a = run("A")
                b = run("B")
                ta.append(a[0])
                te.append(a[1])
                tb.append(b[0])
                delta = max(delta, max_delta(a[2], b[2]))
            spread = float(np.max(ta) - np.min(ta))
            print(json.dumps(dict(shape=shape, candidates=Cn, iters=args.iters, reps=args.reps,
                                  a_ms_per_iter_median=float(np.median(ta)), a_min=float(np.min(ta)),
                                  a_max=float(np.max(ta)), a_spread=spread,
                                  a_expand_ms_per_iter_median=float(np.median(te)),
                                  b_ms_per_iter_median=float(np.median(tb)), b_min=float(np.min(tb)),
                                  b_max=float(np.max(tb)), a_over_b=float(np.median(ta) / np.median(tb)),
                                  b_not_above_a_plus_spread=bool(np.median(tb) <= np.median(ta) + spread),
                                  node_changes_per_iter=a[3], group_changes_per_iter=b[4],
                                  max_abs_delta=delta)), flush=True)


if __name__ == "__main__":
    main()
