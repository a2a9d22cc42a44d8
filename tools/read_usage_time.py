"""Time the per-read usage over mapping lists (phmm_run_with_mapping_read_usage) against today's route to the same
matrix, on the same lists, in ONE process:

  states_scores  phmm_run_with_mapping_states without its values (8 bytes per read leave the device)
  states_host    the states call with its values into host memory (24 bytes per list entry)
  numpy          the reduction of those values on the host: exp, then per read np.unique of its nodes and three
                 np.bincount sums (timed alone, on the values of the states_host call before it)
  usage_handle   the new call: rows into the handle, totals and scores to the host (24 bytes per key + 8 per read)
  usage_export   the new call and the export of its rows to the host (36 bytes per row entry more + 8 per read)

    python tools/read_usage_time.py [--workloads cfg3,rep20] [--reps 7] [--warmup 1]

cfg3 and rep20 are bench.py's workloads; the lists are those of a generate_mappings(None) call.  After `--warmup` rounds
(workspace growth, code objects) the variants take turns `--reps` times with no knob set.  Prints one JSON line per
workload: wall ms of each repetition (host clock around the synchronous call), median, minimum and maximum,
phmm_last_call_stats(2) of the last call of each device variant, the bytes that leave the device, and checksums (taken
outside the timed region) that show the routes computed the same matrix.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def numpy_usage(read_off, pos_off, nodes, sl):
    """today's route behind the states call -> (row_off, keys, usage[., 3])"""
    with np.errstate(under="ignore"):
        prob = np.exp(sl)
    row_off, keys, usage = [0], [], []
    for r in range(read_off.size - 1):
        a0, a1 = int(pos_off[read_off[r]]), int(pos_off[read_off[r + 1]])
        k, inv = np.unique(nodes[a0:a1], return_inverse=True)
        keys.append(k)
        usage.append(np.stack([np.bincount(inv, weights=prob[a0:a1, s], minlength=k.size) for s in range(3)], axis=1))
        row_off.append(row_off[-1] + k.size)
    return np.array(row_off, dtype=np.uint64), np.concatenate(keys), np.concatenate(usage)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="cfg3,rep20")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
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
        po, nd, _ = mp.arrays()
        po, off = po.astype(np.int64), rc.offsets.astype(np.int64)
        R, te, tb, N = len(reads), int(po[-1]), int(off[-1]), int(arrays.n_nodes)
        held = {}

        def states_scores():
            return gm.run_with_mapping_states(rc, mp, want_states=False, want_best=False)

        def states_host():
            held["sl"] = gm.run_with_mapping_states(rc, mp, want_best=False)[1]
            return None

        def numpy():
            return numpy_usage(off, po, nd, held["sl"])

        def usage_handle():
            return gm.run_with_mapping_read_usage(rc, mp)

        def usage_export():
            lf, u = gm.run_with_mapping_read_usage(rc, mp)
            u.arrays()
            return lf, u

        runs = [("states_scores", states_scores), ("states_host", states_host), ("numpy", numpy),
                ("usage_handle", usage_handle), ("usage_export", usage_export)]

        def timed(v, fn):
            t0 = time.perf_counter()
            out = fn()
            ms = (time.perf_counter() - t0) * 1e3
            st = _ffi.last_call_stats(2)
            return ms, out, None if v == "numpy" else {"ms": round(st[0], 3), "launches": int(st[1]), "cells": int(st[2])}

        for _ in range(args.warmup):
            for v, fn in runs:
                timed(v, fn)
        ms = {v: [] for v, _ in runs}
        last, sums, rows = {}, {}, 0
        for rep in range(args.reps):
            for v, fn in runs:
                t, out, st = timed(v, fn)
                ms[v].append(round(t, 3))
                last[v] = st
                if rep + 1 == args.reps:
                    if v == "numpy":
                        sums[v] = [int(out[1].size), int(out[1].astype(np.uint64).sum()), float(out[2].sum())]
                    elif v == "usage_export":
                        row_off, keys, usage = out[1].arrays()
                        rows = int(keys.size)
                        sums[v] = [rows, int(keys.astype(np.uint64).sum()), float(usage.sum()), float(out[1].totals.sum())]
                del out
            print(f"{name}: round {rep + 1} of {args.reps}: " + ", ".join(f"{v} {ms[v][-1]:.1f}" for v, _ in runs),
                  file=sys.stderr, flush=True)
        med ={v: float(np.median(x)) for v, x in ms.items()}
        print(json.dumps({
            "workload": name, "reads": R, "n_nodes": N, "bases": tb, "list_entries": te, "row_entries": rows,
            "keys_per_base": round(rows / max(tb, 1), 3),
            "bytes_off_device": {"states_scores": 8 * R, "states_host": 24 * te + 8 * R, "usage_handle": 24 * N + 8 * R,
                                 "usage_export": 24 * N + 8 * R + 36 * rows + 8 * (R + 1)},
            "ms": ms,
            "median_min_max": {v: [round(med[v], 3), min(x), max(x)] for v, x in ms.items()},
            "todays_route_median_ms": round(med["states_host"] + med["numpy"], 3),
            "stats2": last, "checksums (row entries, sum of keys, sum of usage[, sum of totals])": sums}), flush=True)
        # the next workload's adaptive pass plans with all the memory the device has: give this one's back first
        held.clear()
        del gm, rc, mp
        L.phmm_release_workspace()


if __name__ == "__main__":
    main()
