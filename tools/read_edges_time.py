"""Time the per-read transition usage over mapping lists (phmm_run_with_mapping_read_edges) against the summed call it
shares its list pass with, on the same lists, in ONE process:

  edge_freqs     (a) run_with_mapping_edge_freqs: the records summed over all reads (the baseline)
  edges_handle   (b) the new call: rows into the handle; scores, end terms and totals to the host
  edges_export   (c) the new call and the export of its rows to the host (12 bytes per row entry + 8 per read more)
  reduce_device  (d) the reduction's device time: index 2 of phmm_last_call_stats of the (b) calls

    python tools/read_edges_time.py [--workloads cfg3,rep20] [--reps 7] [--warmup 1] [--out profiles/read_edges.txt]

cfg3 and rep20 are bench.py's workloads; the lists are those of a generate_mappings(None) call.  After `--warmup` rounds
(workspace growth, code objects) the variants take turns `--reps` times with no knob set.  Prints one JSON line per
workload and appends it to `--out`: wall ms of each repetition (host clock around the synchronous call), median, minimum
and maximum, the ratio (b) / (a) of the medians with the extreme ratios the repetitions allow, the statistics of the
last (b) call, the bytes that leave the device, and checksums (taken outside the timed region) that tie the rows to the
summed call's output.  No threshold: these are first numbers.
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
    ap.add_argument("--workloads", default="cfg3,rep20")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "read_edges.txt"))
    args = ap.parse_args()
    import bench
    import dbgphmm_amd as D
    from dbgphmm_amd import _ffi
    L = _ffi.lib()
    _ffi.check(L.phmm_set_device(0))
    L.phmm_enable_timing(1)

    for name in args.workloads.split(","):
        arrays, reads, _ = bench.build_workload(name)
        gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
        mp, _ = gm.generate_mappings(rc, None, True)
        R, E, N, tb = len(reads), int(arrays.n_edges), int(arrays.n_nodes), int(rc.offsets[-1])
        te = int(mp.arrays()[0][-1])

        def edge_freqs():
            return gm.run_with_mapping_edge_freqs(rc, mp)

        def edges_handle():
            return gm.run_with_mapping_read_edges(rc, mp)

        def edges_export():
            lf, u = gm.run_with_mapping_read_edges(rc, mp)
            u.arrays()
            return lf, u

        runs = [("edge_freqs", edge_freqs), ("edges_handle", edges_handle), ("edges_export", edges_export)]

        def timed(fn):
            t0 = time.perf_counter()
            out = fn()
            ms = (time.perf_counter() - t0) * 1e3
            st = _ffi.last_call_stats(2)
            return ms, out, {"ms": round(st[0], 3), "launches": int(st[1]), "cells": int(st[2])}

        for _ in range(args.warmup):
            for _, fn in runs:
                timed(fn)
        ms = {v: [] for v, _ in runs}
        ms["reduce_device"] = []
        last, sums, rows = {}, {}, 0
        for rep in range(args.reps):
            for v, fn in runs:
                t, out, st = timed(fn)
                ms[v].append(round(t, 3))
                last[v] = st
                if v == "edges_handle":
                    ms["reduce_device"].append(st["ms"])
                if rep + 1 == args.reps:
                    if v == "edge_freqs":
                        sums[v] = [float(out[1].sum()), float(out[2].sum())]
                    elif v == "edges_export":
                        row_off, keys, usage = out[1].arrays()
                        rows = int(keys.size)
                        sums[v] = [rows, int(keys.astype(np.uint64).sum()), float(usage.sum()), float(out[1].totals[:E].sum()),
                                   float(out[1].totals[E:].sum())]
                del out
            print(f"{name}: round {rep + 1} of {args.reps}: " + ", ".join(f"{v} {x[-1]:.1f}" for v, x in ms.items()),
                  file=sys.stderr, flush=True)
        med = {v: float(np.median(x)) for v, x in ms.items()}
        a, b = ms["edge_freqs"], ms["edges_handle"]
        line = json.dumps({
            "workload": name, "reads": R, "n_nodes": N, "n_edges": E, "bases": tb, "list_entries": te,
            "records": last["edges_handle"]["cells"], "row_entries": rows, "keys_per_base": round(rows / max(tb, 1), 3),
            "bytes_off_device": {"edge_freqs": 8 * (E + N + R), "edges_handle": 8 * (E + N) + 24 * R,
                                 "edges_export": 8 * (E + N) + 24 * R + 12 * rows + 8 * (R + 1)},
            "ms": ms,
            "median_min_max": {v: [round(med[v], 3), min(x), max(x)] for v, x in ms.items()},
            "handle_over_edge_freqs": {"of_medians": round(med["edges_handle"] / med["edge_freqs"], 4),
                                       "least (min b / max a)": round(min(b) / max(a), 4),
                                       "most (max b / min a)": round(max(b) / min(a), 4)},
            "stats2_of_the_last_call": last,
            "checksums (edge_freqs: sum ef, sum inf; export: row entries, sum of keys, sum of usage, sum totals[:E], "
            "sum totals[E:] without end terms)": sums})
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        # the next workload's adaptive pass plans with all the memory the device has: give this one's back first
        del gm, rc, mp
        L.phmm_release_workspace()


if __name__ == "__main__":
    main()
