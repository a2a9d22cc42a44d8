"""Time the hinted forward on a tandem repeat (bench workload `rep20`: nearly every read's longest mapping list holds
65-400 nodes) with the library PHMM_AMD_LIB names -- the same process runs either side of an A/B comparison (the wide
class of this library is opt-in: PHMM_WIDE_HINTED=1 on its side):

  full    one hinted to_full_prob_reads call (one candidate: the model's own probabilities)
  search  a greedy search on the likelihood handle: per iteration score C candidates given as changes to the current
          vector (16 random k-mers +-1 each, totals only), move to the best

    PHMM_AMD_LIB=/path/to/libphmm_amd.so python tools/hinted_wide_time.py [--workload rep20] [--cands 64] [--iters 20]
                                                                          [--reps 3]

One process per side, the sides alternated by the caller (parent commit's library, this one, ...), as
tools/r3_ab_bench.sh does; the mappings are generated once per process.  Prints one JSON line: wall ms of each
repetition (host clock around the synchronous calls), their median, and phmm_last_call_stats(4) of the last full call
when the library has that class.  Checksums (sum of ln P, the totals of the last iteration) show that both sides
computed the same thing.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="rep20")
    ap.add_argument("--cands", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import bench
    import dbgphmm_amd as D
    from dbgphmm_amd import _ffi
    L = _ffi.lib()
    _ffi.check(L.phmm_set_device(0))
    L.phmm_enable_timing(1)
    arrays, reads, w = bench.build_workload(args.workload)
    sg = bench.cfg_seq_graph(args.workload)
    gm1, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    mp, _ = gm1.generate_mappings(rc, None, True)
    gm = D.PHMMModel(D.vectorised_to_phmm(sg, arrays.param, 0))
    base = sg.copy_num.astype(np.uint32)

    def stats4():
        ms, n, c = C.c_double(), C.c_uint64(), C.c_uint64()
        if L.phmm_last_call_stats(4, C.byref(ms), C.byref(n), C.byref(c)) != 0:
            return None
        return {"ms": ms.value, "launches": n.value, "cells": c.value}

    def full():
        t0 = time.perf_counter()
        tot, _ = gm.to_full_prob_reads(rc, mp)
        return (time.perf_counter() - t0) * 1e3, tot

    def search():
        lk = gm.likelihood(rc, mp, base, 0)
        vec = base.copy()
        t0 = time.perf_counter()
        for it in range(args.iters):
            rng = np.random.default_rng(1000 + it)
            chs = []
            for _ in range(args.cands):
                ix = np.unique(rng.integers(0, vec.size, size=16))
                chs.append((ix, np.maximum(vec[ix].astype(np.int64) + rng.choice([-1, 1], size=ix.size), 0)))
            off = np.zeros(len(chs) + 1, np.uint64)
            off[1:] = np.cumsum([n.size for n, _ in chs])
            node = np.concatenate([n for n, _ in chs]).astype(np.uint32)
            cn = np.concatenate([v for _, v in chs]).astype(np.uint32)
            tot, _, _ = lk.score_changes((off, node, cn), per_read=False)
            best = int(np.argmax(tot))
            lk.move(chs[best][0].astype(np.uint32), chs[best][1].astype(np.uint32))
            vec[chs[best][0]] = chs[best][1]
        return (time.perf_counter() - t0) * 1e3 / args.iters, float(tot[best])

    full()
    search()  # warm-up: workspace growth
    f = [full() for _ in range(args.reps)]
    s4 = stats4()
    s = [search() for _ in range(args.reps)]
    print(json.dumps({
        "lib": _ffi.LIB_PATH, "workload": args.workload, "reads": len(reads), "n_nodes": int(base.size),
        "full_ms": [round(x[0], 3) for x in f], "full_ms_median": round(float(np.median([x[0] for x in f])), 3),
        "full_sum_lnP": f[-1][1], "stats4_full": s4,
        "search_ms_per_iter": [round(x[0], 3) for x in s],
        "search_ms_per_iter_median": round(float(np.median([x[0] for x in s])), 3),
        "search_last_total": s[-1][1], "cands": args.cands, "iters": args.iters}), flush=True)


if __name__ == "__main__":
    main()
