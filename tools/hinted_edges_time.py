"""Time the transition posteriors over mapping lists (phmm_run_with_mapping_edges) against the hinted mapping call
they mirror (phmm_generate_mappings with the same mappings), in one process.

Per workload, in a process of its own: generate_mappings(None) once for the lists, both calls warmed up, then `--reps`
rounds that alternate them.  Prints one JSON line per workload (median and min ms of each call, their ratio, the list
shape).

    python tools/hinted_edges_time.py [--workloads cfg3,rep20] [--reps 5] [--warmup 2]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (workload builders only)
import dbgphmm_amd as D  # noqa: E402


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="cfg3,rep20")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    names = args.workloads.split(",")
    if len(names) > 1:  # (one process per workload: the device pool of one does not shape the next)
        for name in names:
            subprocess.run([sys.executable, os.path.abspath(__file__), "--workloads", name, "--reps", str(args.reps),
                            "--warmup", str(args.warmup)], check=True)
        return
    for name in names:
        arrays, reads, w = bench.build_workload(name)
        model = D.PHMMModel(arrays)
        rc = D.ReadCollection(reads)
        mp, _ = model.generate_mappings(rc, None, True)
        po = mp.arrays()[0].astype(np.int64)
        nf = np.empty(arrays.n_nodes)

        def hinted():
            return model.generate_mappings(rc, mp, True, out_node_freq=nf)

        def edges():
            return model.run_with_mapping_edge_freqs(rc, mp)
        for _ in range(args.warmup):
            hinted()
            edges()
        th, te = [], []
        for _ in range(args.reps):
            t, _ = timed(hinted)
            th.append(t)
            t, (lf, ef, inf) = timed(edges)
            te.append(t)
        line = dict(workload=name, reads=len(reads), bases=int(rc.offsets[-1]), n_nodes=arrays.n_nodes,
                    n_edges=arrays.n_edges, mean_list=float(np.diff(po).mean()), max_list=int(np.diff(po).max()),
                    hinted_ms_median=float(np.median(th)), hinted_ms_min=float(np.min(th)),
                    edges_ms_median=float(np.median(te)), edges_ms_min=float(np.min(te)),
                    ratio_median=float(np.median(te) / np.median(th)), reps=args.reps,
                    init_freq_sum=float(inf.sum()), edge_freq_sum=float(ef.sum()))
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
