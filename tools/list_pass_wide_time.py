"""Time the list pass (run_with_mapping: forward_with_mapping with stored columns + backward_with_mapping) with the wide
classes on a block switched off and on, in ONE process:

  lists   generate_mappings(reads, mappings, use_max_ratio = True) on the lists of a generate_mappings(None) call
  edges   run_with_mapping_edge_freqs on the same lists

    python tools/list_pass_wide_time.py [--workloads rep20,cfg3,u100] [--reps 7] [--warmup 2] [--coverage 20]

rep20 and cfg3 are bench.py's workloads; u100 and u20 are tests/repeat_cases.py's data sets of those names at k = 40 (a
100 bp unit x 10 and a 20 bp unit x 50: the short lists of wide reads, the range of the 128-thread backward block);
--coverage is their read depth (20 as the tests build them: 79 reads; 1000: some 4000 reads, more blocks than a device holds).

Per workload and call, after `--warmup` calls of every variant (workspace growth, code objects), the variants take turns
`--reps` times: `off` (PHMM_NO_WIDE_HINTED=1: the generic one-wave kernels, the default's launches), `fwd`
(PHMM_WIDE_HINTED=1 PHMM_NO_WIDE_LIST_BWD=1: block forward, generic backward), `on` (lists: PHMM_WIDE_HINTED=1, both
halves on the block; for `edges` that is `fwd`, left out), `edges_on` (edges: PHMM_WIDE_HINTED=1 PHMM_WIDE_EDGE_BWD=1,
both halves on the block) and `on128` / `on448` (both halves on the block with PHMM_WIDE_BWD_T=128 / 448: the backward
block's size for reads whose longest list holds at most 128 nodes).  The knobs are read at every call.  Prints one JSON
line per workload and call: the spread of the longest list per read (which block size a read takes), wall ms of each
repetition per variant (host clock around the synchronous call), median, minimum and maximum, phmm_last_call_stats(4) of
the last call of each variant, and checksums that show every variant computed the same thing.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

VARIANTS = {
    "off": {"PHMM_NO_WIDE_HINTED": "1"},
    "fwd": {"PHMM_WIDE_HINTED": "1", "PHMM_NO_WIDE_LIST_BWD": "1"},
    "on": {"PHMM_WIDE_HINTED": "1"},
    "edges_on": {"PHMM_WIDE_HINTED": "1", "PHMM_WIDE_EDGE_BWD": "1"},
    "on128": {"PHMM_WIDE_HINTED": "1", "PHMM_WIDE_EDGE_BWD": "1", "PHMM_WIDE_BWD_T": "128"},
    "on448": {"PHMM_WIDE_HINTED": "1", "PHMM_WIDE_EDGE_BWD": "1", "PHMM_WIDE_BWD_T": "448"},
}
KNOBS = ("PHMM_WIDE_HINTED", "PHMM_NO_WIDE_HINTED", "PHMM_NO_WIDE_LIST_BWD", "PHMM_WIDE_EDGE_BWD", "PHMM_WIDE_BWD_T")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="rep20,cfg3")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--coverage", type=int, default=20, help="read depth of the u100 / u20 data sets")
    args = ap.parse_args()
    import bench
    import dbgphmm_amd as D
    from dbgphmm_amd import _ffi
    L = _ffi.lib()
    _ffi.check(L.phmm_set_device(0))
    L.phmm_enable_timing(1)

    def under(variant, fn):
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(VARIANTS[variant])
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
        if name in ("u100", "u20"):
            sys.path.insert(0, os.path.join(HERE, "tests"))
            from repeat_cases import dataset
            arrays, reads, _, _ = dataset(name, 40, coverage=args.coverage)
        else:
            arrays, reads, _ = bench.build_workload(name)
        gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
        for k in KNOBS:
            os.environ.pop(k, None)
        mp, _ = gm.generate_mappings(rc, None, True)
        po = mp.arrays()[0].astype(np.int64)
        off = rc.offsets.astype(np.int64)
        rmax = np.array([np.diff(po[off[r]:off[r + 1] + 1]).max(initial=0) for r in range(len(reads))])

        def lists():
            out, nf = gm.generate_mappings(rc, mp, True)
            return [float(out.read_logp()[0]), float(out.read_logp_backward()[0]), float(nf.sum())]

        def edges():
            lf, ef, inf = gm.run_with_mapping_edge_freqs(rc, mp)
            return [float(lf.sum()), float(ef.sum()), float(inf.sum())]

        for call, fn, variants in (("lists", lists, ("off", "fwd", "on", "on128", "on448")),
                                   ("edges", edges, ("off", "fwd", "edges_on", "on128", "on448"))):
            for _ in range(args.warmup):
                for v in variants:
                    under(v, fn)
            ms = {v: [] for v in variants}
            last = {}
            for _ in range(args.reps):
                for v in variants:
                    t, out, st = under(v, fn)
                    ms[v].append(round(t, 3))
                    last[v] = {"checksums": out, "stats4": st}
            print(json.dumps({
                "workload": name, "call": call, "reads": len(reads), "n_nodes": int(arrays.n_nodes),
                "reads_with_lists_65_400": int(((rmax > 64) & (rmax <= 400)).sum()), "list_entries": int(po[-1]),
                "read_max_list": {"min": int(rmax.min()), "median": float(np.median(rmax)), "max": int(rmax.max()),
                                  "at_most_64": int((rmax <= 64).sum()), "65_128": int(((rmax > 64) & (rmax <= 128)).sum()),
                                  "129_400": int(((rmax > 128) & (rmax <= 400)).sum())},
                "ms": ms,
                "median_min_max": {v: [round(float(np.median(x)), 3), min(x), max(x)] for v, x in ms.items()},
                "last": last}), flush=True)


if __name__ == "__main__":
    main()
