"""Time the alignment records (phmm_run_with_mapping_alignments, exported to host memory) at n_samples 0, 1, 8 and 64
against the parent calls over the same lists, in ONE process:

  align_S       run_with_mapping_alignments, n_samples = S (0: the best path), then Alignments.arrays(): the records in
                host memory
  rows_S        the parent call -- run_with_mapping_best_path for S = 0, run_with_mapping_sample_paths otherwise -- with
                out_path in host memory: what a user pays for the paths today
  null_S        the parent call with out_path = NULL: the floor (scores and counts only)

    python tools/alignments_time.py [--workloads rep20,cfg3] [--reps 7] [--warmup 2] [--samples 0,1,8,64]

cfg3 and rep20 are bench.py's workloads; the lists are those of a generate_mappings(None) call.  After `--warmup` calls of
everything (workspace growth, code objects) the calls take turns `--reps` times, no knob set.  Prints one JSON line per
workload: wall ms of each repetition (host clock around the synchronous call and the export), median, minimum and
maximum, phmm_last_call_stats(2) of the last calls, and per S the bytes of the compact records (both offset arrays, the
CIGAR words, the walk runs) against the bytes of the rows (4 (n_max_gaps + 2) S' per base), with the mean CIGAR words
and walk runs per alignment.
PHMM_TRACE=1 prints the host-side phase times of every call on stderr ("alignments count", "alignments scan",
"alignments write" beside the parent's "forward" and "walk" / "traceback" marks).
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
    ap.add_argument("--samples", default="0,1,8,64")
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
        out, st = fn()
        ms = (time.perf_counter() - t0) * 1e3
        return ms, out, {"ms": round(st[0], 3), "launches": int(st[1]), "cells": int(st[2])}

    for name in args.workloads.split(","):
        arrays, reads, _ = bench.build_workload(name)
        gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
        mp, _ = gm.generate_mappings(rc, None, True)
        po = mp.arrays()[0].astype(np.int64)
        stride = int(arrays.param.n_max_gaps) + 2
        sizes = {}

        def align(n):
            def run():
                lp, plp, counts, al = gm.run_with_mapping_alignments(rc, mp, n, args.seed)
                st = _ffi.last_call_stats(2)
                op_off, ops, run_off, rn, rl = al.arrays()
                sizes[n] = {"alignments": len(al), "cigar_words": int(ops.size), "walk_runs": int(rn.size),
                            "compact_bytes": int(op_off.nbytes + run_off.nbytes + ops.nbytes + rn.nbytes + rl.nbytes),
                            "row_bytes": 4 * stride * rc.total_bases() * max(n, 1)}
                return [float(lp[np.isfinite(lp)].sum()), int(counts.astype(np.int64).sum()), int(ops.size), int(rn.size)], st
            return run

        def parent(n, want_path):
            def run():
                if n == 0:
                    lp, path, counts = gm.run_with_mapping_best_path(rc, mp, want_path=want_path)
                else:
                    lp, _, path, counts, _ = gm.run_with_mapping_sample_paths(rc, mp, n, args.seed, want_path=want_path)
                st = _ffi.last_call_stats(2)
                out = [float(lp[np.isfinite(lp)].sum()), int(counts.astype(np.int64).sum())]
                if want_path:
                    out.append(int((path[..., 1:] != D.PATH_NONE).sum()))
                return out, st
            return run

        runs = []
        for n in samples:
            runs += [(f"align_{n}", align(n)), (f"rows_{n}", parent(n, True)), (f"null_{n}", parent(n, False))]
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
        for n, z in sizes.items():
            z["compact_over_rows"] = round(z["compact_bytes"] / max(z["row_bytes"], 1), 5)
            z["cigar_words_per_alignment"] = round(z["cigar_words"] / max(z["alignments"], 1), 2)
            z["walk_runs_per_alignment"] = round(z["walk_runs"] / max(z["alignments"], 1), 2)
        print(json.dumps({
            "workload": name, "reads": len(reads), "n_nodes": int(arrays.n_nodes), "bases": int(rc.total_bases()),
            "list_entries": int(po[-1]), "stride": stride, "ms": ms,
            "median_min_max": {v: [round(float(np.median(x)), 3), min(x), max(x)] for v, x in ms.items()},
            "sizes": {str(n): z for n, z in sizes.items()}, "last": last}), flush=True)
        # the next workload's adaptive pass plans with all the memory the device has: give this one's back first
        del gm, rc, mp
        L.phmm_release_workspace()


if __name__ == "__main__":
    main()
