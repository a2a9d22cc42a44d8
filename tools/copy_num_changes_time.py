"""Time candidates given as changes to a base vector (phmm_full_prob_reads_copy_num_changes) against the full form on
the materialised vectors (phmm_full_prob_reads_copy_nums), in one process, on cfg3.

Two candidate shapes: bench's (`--mode candidates`: 16 random k-mers +-1, seed 5, candidate 0 = the base) and bubble
swaps (between two k-mers both haplotypes share, the hap-A-only k-mers +1 and the hap-B-only k-mers -1).  Per case
both calls are warmed up, then `--reps` rounds alternate them, each timed with a host clock around the synchronous
call.  Prints one JSON line per case: ms of each form (median, min), the speed-up, the rescored share, and the largest
per-read |delta| between the two forms.

    python tools/copy_num_changes_time.py [--cands 64,256,1024] [--reps 5] [--warmup 2] [--shapes bench,bubble]
"""
import argparse
import json
import os
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


def bench_shape(base, C):
    rng = np.random.default_rng(5)
    cn = np.repeat(base[None, :], C, axis=0)
    for c in range(1, C):
        ix = rng.integers(0, base.size, size=16)
        cn[c, ix] = np.maximum(cn[c, ix].astype(np.int64) + rng.choice([-1, 1], size=16), 0).astype(np.uint32)
    return cn


def bubbles(sg, occ):
    a, b = occ
    in_a, in_b = np.zeros(sg.base.size, bool), np.zeros(sg.base.size, bool)
    in_a[a] = True
    in_b[b] = True
    pos_b = {int(v): i for i, v in enumerate(b)}
    shared = np.flatnonzero(in_b[a])
    out = []
    for i in range(shared.size - 1):
        lo, hi = shared[i], shared[i + 1]
        if hi - lo < 3 or int(a[lo]) not in pos_b or int(a[hi]) not in pos_b:
            continue
        ib, jb = pos_b[int(a[lo])], pos_b[int(a[hi])]
        if jb <= ib:
            continue
        a_only = np.unique(a[lo + 1:hi][~in_b[a[lo + 1:hi]]])
        b_only = np.unique(b[ib + 1:jb][~in_a[b[ib + 1:jb]]])
        if a_only.size and b_only.size:
            out.append((a_only, b_only))
    return out


def bubble_shape(base, swaps, C):
    cn = np.repeat(base[None, :], C, axis=0)
    for c in range(1, C):
        a_only, b_only = swaps[(c - 1) % len(swaps)]
        cn[c, a_only] += 1
        cn[c, b_only] = np.maximum(cn[c, b_only].astype(np.int64) - 1, 0).astype(np.uint32)
    return cn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cands", default="64,256,1024")
    ap.add_argument("--shapes", default="bench,bubble")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    arrays, reads, w = bench.build_workload("cfg3")
    sg, occ = D.dbg_from_haplotypes(bench.cfg_haplotypes("cfg3"), w["k"], with_occurrences=True)
    model = D.PHMMModel(arrays)
    rc = D.ReadCollection(reads)
    mp, _ = model.generate_mappings(rc, None, True)
    base = sg.copy_num.astype(np.uint32)
    swaps = bubbles(sg, occ)
    for shape in args.shapes.split(","):
        for C in (int(x) for x in args.cands.split(",")):
            cn = bench_shape(base, C) if shape == "bench" else bubble_shape(base, swaps, C)
            changes = D.copy_num_changes(base, cn)

            def full():
                return model.to_full_prob_reads_copy_nums(rc, mp, cn, 0)

            def change():
                return model.to_full_prob_reads_copy_num_changes(rc, mp, base, changes, 0)
            for _ in range(args.warmup):
                full()
                change()
            tf, tc = [], []
            for _ in range(args.reps):
                t, (tot_f, lp_f) = timed(full)
                tf.append(t)
                t, (tot_c, lp_c, nres) = timed(change)
                tc.append(t)
            with np.errstate(invalid="ignore"):
                d = np.where(np.isneginf(lp_f) & np.isneginf(lp_c), 0.0, np.abs(lp_f - lp_c))
                dt = np.where(tot_f == tot_c, 0.0, np.abs(tot_f - tot_c))
            line = dict(workload="cfg3", shape=shape, candidates=C, reads=len(reads), n_nodes=arrays.n_nodes,
                        full_ms_median=float(np.median(tf)), full_ms_min=float(np.min(tf)),
                        change_ms_median=float(np.median(tc)), change_ms_min=float(np.min(tc)),
                        speedup_median=float(np.median(tf) / np.median(tc)),
                        rescored_share=float(nres.sum()) / (C * len(reads)),
                        rescored_share_excl_base=float(nres[1:].sum()) / (max(C - 1, 1) * len(reads)),
                        max_abs_delta=float(np.max(d)),
                        max_abs_delta_total=float(np.max(dt)),
                        reps=args.reps)
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
