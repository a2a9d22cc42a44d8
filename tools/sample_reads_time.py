"""Time reads drawn from the model on the device (phmm_sample_reads through PHMMModel.sample_reads_raw) beside the host
loop graph.sample_reads for the same amount, in ONE process:

  device_null    the call with every output NULL but the lengths (nothing but n_walks words leaves the device)
  device_bases   the same with out_bases in host memory (length + 1 bytes per walk leave the device)
  device_history the same with bases and history words in host memory
  host           graph.sample_reads (lockstep numpy, its own PCG64 stream) for the same number of reads

    python tools/sample_reads_time.py [--workloads cfg3,rep20] [--walks 4026] [--length 1000] [--reps 7] [--warmup 2]
                                      [--out profiles/sample_reads.txt]

cfg3 and rep20 are bench.py's models.  After `--warmup` calls of every form (workspace growth, code objects) the forms
take turns `--reps` times.  Writes one JSON line per workload: wall ms of each repetition (host clock around the
synchronous call), median, minimum and maximum, phmm_last_call_stats(2) of the last call of each device form (device ms,
launches, steps taken), ns per step of a walk (device ms / length: a lane's chain of dependent loads) and per step of
the call (device ms / steps taken), and the flag counts.  PHMM_TRACE=1 prints the host-side phase times on stderr."""
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
    ap.add_argument("--walks", type=int, default=4026)
    ap.add_argument("--length", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "sample_reads.txt"))
    args = ap.parse_args()
    import bench
    import dbgphmm_amd as D
    from dbgphmm_amd import _ffi
    L = _ffi.lib()
    _ffi.check(L.phmm_set_device(0))
    L.phmm_enable_timing(1)
    lines = []
    for name in args.workloads.split(","):
        arrays, _, _ = bench.build_workload(name)
        gm = D.PHMMModel(arrays)
        n, length = args.walks, args.length
        keep = {}

        def timed(fn):
            """fn() makes the call and returns a function that sums its outputs up, outside the clock"""
            t0 = time.perf_counter()
            after = fn()
            ms = (time.perf_counter() - t0) * 1e3
            st = _ffi.last_call_stats(2)
            return ms, after(), {"ms": round(st[0], 3), "launches": int(st[1]), "cells": int(st[2])}

        ln0 = np.empty(n, dtype=np.uint32)

        def device_null():
            _ffi.check(L.phmm_sample_reads(gm._h, 0, n, length, 0, None, 0, args.seed, None, ln0.ctypes.data, None, None, 0,
                                           None, None))
            return lambda: [int(ln0.sum())]

        def device_bases():
            bases, ln, fl, _, _, _ = gm.sample_reads_raw(0, n, length, "state_count", None, args.seed)
            keep["flags"] = fl
            return lambda: [int(ln.sum()), int(bases.sum(dtype=np.int64))]

        def device_history():
            bases, ln, fl, hist, hl, _ = gm.sample_reads_raw(0, n, length, "state_count", None, args.seed, want_history=True)
            return lambda: [int(ln.sum()), int(hl.sum())]

        def host():
            reads = D.sample_reads(arrays, 10 ** 12, length, seed=args.seed, max_reads=n)
            return [sum(len(r) for r in reads)]

        runs = [("device_null", device_null), ("device_bases", device_bases), ("device_history", device_history)]
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
        ms["host"] = []
        for _ in range(args.host_reps):
            t0 = time.perf_counter()
            out = host()
            ms["host"].append(round((time.perf_counter() - t0) * 1e3, 3))
            last["host"] = {"checksums": out}
        st = last["device_null"]["stats2"]
        fl = keep["flags"]
        lines.append(json.dumps({
            "workload": name, "n_nodes": int(arrays.n_nodes), "n_edges": int(arrays.n_edges), "walks": n, "length": length,
            "kind": "state_count", "ms": ms,
            "median_min_max": {v: [round(float(np.median(x)), 3), min(x), max(x)] for v, x in ms.items()},
            "ns_per_step_of_a_walk": round(st["ms"] * 1e6 / length, 1),
            "ns_per_step_of_the_call": round(st["ms"] * 1e6 / max(st["cells"], 1), 3),
            "flags": {"ended": int((fl & 1 != 0).sum()), "dead_end": int((fl & 2 != 0).sum()), "state_cap": int((fl & 4 != 0).sum())},
            "last": last}))
        print(lines[-1], flush=True)
        del gm
        L.phmm_release_workspace()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("tools/sample_reads_time.py: phmm_sample_reads against the host loop graph.sample_reads, one MI355X, one process; "
                "wall ms per call,\nmedians of --reps calls after --warmup (see the tool's docstring for the forms)\n")
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
