"""Time posterior path sampling over mapping lists (phmm_run_with_mapping_sample_paths) at n_samples 1, 8 and 64
against the best path over the same lists (phmm_run_with_mapping_best_path, out_path = NULL: the yardstick), in ONE
process:

  sample_S_null    run_with_mapping_sample_paths, n_samples = S, out_path = NULL (ln Z, the path values and the counts only)
  sample_S         the same with out_path in host memory (4 (n_max_gaps + 2) S bytes per base leave the device)
  best_path_null   run_with_mapping_best_path with out_path = NULL

    python tools/sample_paths_time.py [--workloads rep20,cfg3] [--reps 7] [--warmup 2] [--samples 1,8,64]

cfg3 and rep20 are bench.py's workloads; the lists are those of a generate_mappings(None) call.  After `--warmup` calls of
everything (workspace growth, code objects) the calls take turns `--reps` times, no knob set.  Prints one JSON line per
workload: wall ms of each repetition (host clock around the synchronous call), median, minimum and maximum,
phmm_last_call_stats(2) of the last calls (device ms between the call's first and last launch, launches, cells), the
mean alignment summary of the samples beside the best path's, and the spread of ln P(path) under ln Z.
PHMM_TRACE=1 prints the host-side phase times of every call on stderr ("sample paths forward", "sample paths walk").
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
    ap.add_argument("--samples", default="1,8,64")
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    import bench
    import dbgphmm_amd as D
    from dbgphmm_amd import _ffi
    L = _ffi.lib()
    _ffi.check(L.phmm_set_device(0))
    L.phmm_enable_timing(1)
    samples = [int(x) for x in args.samples.split(",")]

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
        keep = {}

        def sampler(n, want_path):
            def run():
                lp, plp, path, counts, _ = gm.run_with_mapping_sample_paths(rc, mp, n, args.seed, want_path=want_path)
                keep[n] = (lp, plp, counts)
                out = [float(lp.sum()), float(plp.sum()), int(counts.astype(np.int64).sum())]
                if want_path:
                    out.append(int((path[:, :, 1:] != D.PATH_NONE).sum()))
                return out
            return run

        def best_path_null():
            lp, _, counts = gm.run_with_mapping_best_path(rc, mp, want_path=False)
            keep["best"] = (lp, counts)
            return [float(lp.sum()), int(counts.astype(np.int64).sum())]

        runs = [("best_path_null", best_path_null)]
        for n in samples:
            runs += [(f"sample_{n}_null", sampler(n, False)), (f"sample_{n}", sampler(n, True))]
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
        n = samples[-1]
        lp, plp, counts = keep[n]
        ok = np.isfinite(lp)
        under = (lp[ok, None] - plp[ok]).ravel()
        print(json.dumps({
            "workload": name, "reads": len(reads), "n_nodes": int(arrays.n_nodes), "bases": int(off[-1]),
            "list_entries": int(po[-1]), "stride": int(arrays.param.n_max_gaps) + 2, "record_bytes": 128 * int(po[-1]),
            "ms": ms,
            "median_min_max": {v: [round(float(np.median(x)), 3), min(x), max(x)] for v, x in ms.items()},
            "best_path_counts": keep["best"][1].astype(np.int64).sum(axis=0).tolist(),
            f"mean_counts_of_{n}_samples": (counts.astype(np.int64).sum(axis=(0, 1)) / n).tolist(),
            "ln_z_minus_ln_p_path": {"min": float(under.min()), "median": float(np.median(under)), "max": float(under.max())},
            "ln_z_minus_best_path": {"median": float(np.median(lp[ok] - keep["best"][0][ok]))},
            "last": last}), flush=True)
        # the next workload's adaptive pass plans with all the memory the device has: give this one's back first
        del gm, rc, mp
        L.phmm_release_workspace()


if __name__ == "__main__":
    main()
