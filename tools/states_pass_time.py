"""Time the state posteriors over mapping lists (phmm_run_with_mapping_states) against the two other list calls, on the
same lists, in ONE process:

  states       run_with_mapping_states, both outputs (24 bytes per list entry + 4 per base leave the device)
  states_best  run_with_mapping_states with out_state_logp = NULL (4 bytes per base)
  edges        run_with_mapping_edge_freqs
  lists        generate_mappings(reads, mappings, use_max_ratio = True)

    python tools/states_pass_time.py [--workloads rep20,cfg3] [--reps 7] [--warmup 2]

cfg3 and rep20 are bench.py's workloads; the lists are those of a generate_mappings(None) call.  After `--warmup` calls
of everything (workspace growth, code objects) the calls take turns `--reps` times with no knob set (the default's
launches: the generic one-wave kernels).  On rep20, whose reads have lists of 65-400 nodes, the states call is also timed
with PHMM_NO_WIDE_HINTED=1 (`generic`), PHMM_WIDE_HINTED=1 (`fwd`: block forward, generic backward) and
PHMM_WIDE_HINTED=1 PHMM_WIDE_STATES_BWD=1 (`block`: both halves on the block).  Prints one JSON line per workload: wall ms of
each repetition (host clock around the synchronous call), median, minimum and maximum, phmm_last_call_stats(4) of the
last call, and checksums that show the variants computed the same thing.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

KNOBS = ("PHMM_WIDE_HINTED", "PHMM_NO_WIDE_HINTED", "PHMM_NO_WIDE_LIST_BWD", "PHMM_WIDE_EDGE_BWD", "PHMM_WIDE_STATES_BWD",
         "PHMM_WIDE_BWD_T")
BLOCK_VARIANTS = {
    "generic": {"PHMM_NO_WIDE_HINTED": "1"},
    "fwd": {"PHMM_WIDE_HINTED": "1"},
    "block": {"PHMM_WIDE_HINTED": "1", "PHMM_WIDE_STATES_BWD": "1"},
}


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

    def under(setting, fn):
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(setting)
        try:
            t0 = time.perf_counter()
            out = fn()
            ms = (time.perf_counter() - t0) * 1e3
            st = _ffi.last_call_stats(4)
        finally:
            for k in KNOBS:
                os.environ.pop(k, None)
        return ms, out, {"ms": round(st[0], 3), "launches": int(st[1]), "cells": int(st[2])}

    for name in args.workloads.split(","):
        arrays, reads, _ = bench.build_workload(name)
        gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
        for k in KNOBS:
            os.environ.pop(k, None)
        mp, _ = gm.generate_mappings(rc, None, True)
        po = mp.arrays()[0].astype(np.int64)
        off = rc.offsets.astype(np.int64)
        rmax = np.array([np.diff(po[off[r]:off[r + 1] + 1]).max(initial=0) for r in range(len(reads))])

        def states():
            lf, sl, best = gm.run_with_mapping_states(rc, mp)
            return [float(lf.sum()), float(np.exp(sl).sum()), int(best.astype(np.uint64).sum())]

        def states_best():
            lf, _, best = gm.run_with_mapping_states(rc, mp, want_states=False)
            return [float(lf.sum()), int(best.astype(np.uint64).sum())]

        def edges():
            lf, ef, inf = gm.run_with_mapping_edge_freqs(rc, mp)
            return [float(lf.sum()), float(ef.sum()), float(inf.sum())]

        def lists():
            out, nf = gm.generate_mappings(rc, mp, True)
            return [float(out.read_logp()[0]), float(out.read_logp_backward()[0]), float(nf.sum())]

        runs = [("states", {}, states), ("states_best", {}, states_best), ("edges", {}, edges), ("lists", {}, lists)]
        if name == "rep20":
            for v, setting in BLOCK_VARIANTS.items():
                runs.append(("states_" + v, setting, states))
                runs.append(("states_best_" + v, setting, states_best))
        for _ in range(args.warmup):
            for _, setting, fn in runs:
                under(setting, fn)
        ms = {v: [] for v, _, _ in runs}
        last = {}
        for _ in range(args.reps):
            for v, setting, fn in runs:
                t, out, st = under(setting, fn)
                ms[v].append(round(t, 3))
                last[v] = {"checksums": out, "stats4": st}
        print(json.dumps({
            "workload": name, "reads": len(reads), "n_nodes": int(arrays.n_nodes), "bases": int(off[-1]),
            "list_entries": int(po[-1]),
            "read_max_list": {"min": int(rmax.min()), "median": float(np.median(rmax)), "max": int(rmax.max()),
                              "at_most_64": int((rmax <= 64).sum()), "65_400": int(((rmax > 64) & (rmax <= 400)).sum())},
            "ms": ms,
            "median_min_max": {v: [round(float(np.median(x)), 3), min(x), max(x)] for v, x in ms.items()},
            "last": last}), flush=True)
        # the next workload's adaptive pass plans with all the memory the device has: give this one's back first
        del gm, rc, mp
        L.phmm_release_workspace()


if __name__ == "__main__":
    main()
