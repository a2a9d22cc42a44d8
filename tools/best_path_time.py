"""Time the best path over mapping lists (phmm_run_with_mapping_best_path) against the state posteriors over the same
lists (phmm_run_with_mapping_states), in ONE process:

  best_path        run_with_mapping_best_path, out_path in host memory (4 (n_max_gaps + 2) bytes per base leave the device)
  best_path_null   the same with out_path = NULL (ln P and the counts only)
  states_best      run_with_mapping_states with out_state_logp = NULL (the yardstick: a forward and a backward list pass,
                   4 bytes per base leave the device)
  states           run_with_mapping_states, both outputs (24 bytes per list entry leave the device)

    python tools/best_path_time.py [--workloads rep20,cfg3] [--reps 7] [--warmup 2]

cfg3 and rep20 are bench.py's workloads; the lists are those of a generate_mappings(None) call.  After `--warmup` calls of
everything (workspace growth, code objects) the calls take turns `--reps` times, no knob set.  Prints one JSON line per
workload: wall ms of each repetition (host clock around the synchronous call), median, minimum and maximum,
phmm_last_call_stats(2) of the last best-path calls (device ms between the call's first and last launch, launches,
cells), the alignment summary over all reads, and the gap between the forward total and the best path.
PHMM_TRACE=1 prints the host-side phase times of every call on stderr ("best path forward", "best path traceback").
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="rep20,cfg3")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import bench
    import dbgphmm_amd as D
    from dbgphmm_amd import _ffi
    L = _ffi.lib()
    _ffi.check(L.phmm_set_device(0))
    L.phmm_enable_timing(1)

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        ms = (time.perf_counter() - t0) * 1e3
        st = _ffi.last_call_stats(2)
        return ms, out, {"ms": round(st[0], 3), "launches": int(st[1]), "cells": int(st[2])}

    for name in args.workloads.split(","):
        arrays, reads, _ = bench.build_workload(name)
        gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
        mp, _ = gm.generate_mappings(rc, None, True)
        po = mp.arrays()[0].astype(np.int64)
        off = rc.offsets.astype(np.int64)
        rmax = np.array([np.diff(po[off[r]:off[r + 1] + 1]).max(initial=0) for r in range(len(reads))])
        keep = {}

        def best_path():
            lp, path, counts = gm.run_with_mapping_best_path(rc, mp)
            keep["lp"], keep["counts"] = lp, counts
            return [float(lp.sum()), int(counts.astype(np.int64).sum()), int((path[:, 1:] != D.PATH_NONE).sum())]

        def best_path_null():
            lp, _, counts = gm.run_with_mapping_best_path(rc, mp, want_path=False)
            return [float(lp.sum()), int(counts.astype(np.int64).sum())]

        def states_best():
            lf, _, best = gm.run_with_mapping_states(rc, mp, want_states=False)
            keep["lf"] = lf
            return [float(lf.sum()), int(best.astype(np.uint64).sum())]

        def states():
            lf, sl, best = gm.run_with_mapping_states(rc, mp)
            return [float(lf.sum()), int(best.astype(np.uint64).sum())]

        runs = [("best_path", best_path), ("best_path_null", best_path_null), ("states_best", states_best), ("states", states)]
        for _ in range(args.warmup):
            for _, fn in runs:
                timed(fn)
        ms = {v: [] for v, _ in runs}
        last = {}
        for _ in range(args.reps):
            for v, fn in runs:
                t, out, st = timed(fn)
                ms[v].append(round(t, 3))
                last[v] = {"checksums": out, "stats2": st}
        gap = keep["lf"] - keep["lp"]
        print(json.dumps({
            "workload": name, "reads": len(reads), "n_nodes": int(arrays.n_nodes), "bases": int(off[-1]),
            "list_entries": int(po[-1]), "stride": int(arrays.param.n_max_gaps) + 2,
            "read_max_list": {"median": float(np.median(rmax)), "max": int(rmax.max()),
                              "at_most_64": int((rmax <= 64).sum()), "65_400": int(((rmax > 64) & (rmax <= 400)).sum())},
            "ms": ms,
            "median_min_max": {v: [round(float(np.median(x)), 3), min(x), max(x)] for v, x in ms.items()},
            "counts_match_mismatch_ins_del": keep["counts"].astype(np.int64).sum(axis=0).tolist(),
            "forward_minus_best_path": {"min": float(gap.min()), "median": float(np.median(gap)), "max": float(gap.max())},
            "last": last}), flush=True)
        # the next workload's adaptive pass plans with all the memory the device has: give this one's back first
        del gm, rc, mp
        L.phmm_release_workspace()


if __name__ == "__main__":
    main()
