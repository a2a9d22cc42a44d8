"""Time the pileup over mapping lists (phmm_run_with_mapping_pileup) against the parent's route to the same figures and
against its sibling, on the same lists, in ONE process:

  (a) parent         phmm_run_with_mapping_states with its values into host memory (24 bytes per list entry), then the
                     reduction on the host by (node, read base): exp, the position and base of every entry, per read
                     np.unique of its keys and three np.bincount sums, and the [N, 9] totals -- the two parts timed
                     together and apart
  (b) usage_handle   phmm_run_with_mapping_read_usage into the handle with its totals: the sibling of the same flow
  (c) pileup_handle  the new call: rows into the handle, totals and scores to the host (72 bytes per node + 8 per read)
  (d) pileup_export  the new call and the export of its rows to the host (36 bytes per row entry + 8 per read more)

    python tools/pileup_time.py [--workloads cfg3,rep20] [--reps 7] [--warmup 1]

cfg3 and rep20 are bench.py's workloads; the lists are those of a generate_mappings(None) call.  After `--warmup` rounds
(workspace growth, code objects) the variants take turns `--reps` times with no knob set.  Prints one JSON line per
workload: wall ms of each repetition (host clock around the synchronous call), median, minimum and maximum,
phmm_last_call_stats(2) of every repetition of (b) and (c), the bytes that leave the device, whether the ranges of (a)
and (c) overlap, and checksums (taken outside the timed region) that show the routes computed the same matrix.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def numpy_pileup(read_off, bases, pos_off, nodes, sl, n_nodes):
    """the parent's route behind the states call -> (row_off, keys, usage[., 3], totals[N, 9])"""
    with np.errstate(under="ignore"):
        prob = np.exp(sl)
    code = np.full(256, 0, dtype=np.int64)
    code[[ord("C"), ord("G"), ord("T")]] = (1, 2, 3)
    # the position of every entry: empty lists are passed over
    g = np.repeat(np.arange(pos_off.size - 1, dtype=np.int64), np.diff(pos_off))
    key = 4 * nodes.astype(np.int64) + code[bases[g]]
    row_off, keys, usage = [0], [], []
    for r in range(read_off.size - 1):
        a0, a1 = int(pos_off[read_off[r]]), int(pos_off[read_off[r + 1]])
        k, inv = np.unique(key[a0:a1], return_inverse=True)
        keys.append(k)
        usage.append(np.stack([np.bincount(inv, weights=prob[a0:a1, s], minlength=k.size) for s in range(3)], axis=1))
        row_off.append(row_off[-1] + k.size)
    keys, usage = np.concatenate(keys), np.concatenate(usage)
    totals = np.zeros((n_nodes, 9))
    totals[:, 0:4] = np.bincount(keys, weights=usage[:, 0], minlength=4 * n_nodes).reshape(n_nodes, 4)
    totals[:, 4:8] = np.bincount(keys, weights=usage[:, 1], minlength=4 * n_nodes).reshape(n_nodes, 4)
    totals[:, 8] = np.bincount(keys >> 2, weights=usage[:, 2], minlength=n_nodes)
    return np.array(row_off, dtype=np.uint64), keys.astype(np.uint32), usage, totals


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
        split = {}

        def parent():
            t0 = time.perf_counter()
            sl = gm.run_with_mapping_states(rc, mp, want_best=False)[1]
            t1 = time.perf_counter()
            out = numpy_pileup(off, rc.bases, po, nd, sl, N)
            split.setdefault("states_host", []).append(round((t1 - t0) * 1e3, 3))
            split.setdefault("numpy", []).append(round((time.perf_counter() - t1) * 1e3, 3))
            return out

        def usage_handle():
            return gm.run_with_mapping_read_usage(rc, mp)

        def pileup_handle():
            return gm.run_with_mapping_pileup(rc, mp)

        def pileup_export():
            lf, p = gm.run_with_mapping_pileup(rc, mp)
            p.arrays()
            return lf, p

        runs = [("parent", parent), ("usage_handle", usage_handle), ("pileup_handle", pileup_handle),
                ("pileup_export", pileup_export)]

        def timed(v, fn):
            t0 = time.perf_counter()
            out = fn()
            ms = (time.perf_counter() - t0) * 1e3
            st = _ffi.last_call_stats(2)
            return ms, out, round(st[0], 3), int(st[1])

        for _ in range(args.warmup):
            for v, fn in runs:
                timed(v, fn)
        split.clear()
        ms = {v: [] for v, _ in runs}
        dev = {"usage_handle": [], "pileup_handle": []}
        launches, sums, rows, usage_rows = {}, {}, 0, 0
        for rep in range(args.reps):
            for v, fn in runs:
                t, out, dms, nl = timed(v, fn)
                ms[v].append(round(t, 3))
                if v in dev:
                    dev[v].append(dms)
                    launches[v] = nl
                if rep + 1 == args.reps:
                    if v == "parent":
                        sums[v] = [int(out[1].size), int(out[1].astype(np.uint64).sum()), float(out[2].sum()), float(out[3].sum())]
                    elif v == "usage_handle":
                        usage_rows = int(out[1].arrays()[1].size)
                    elif v == "pileup_export":
                        row_off, keys, usage = out[1].arrays()
                        rows = int(keys.size)
                        sums[v] = [rows, int(keys.astype(np.uint64).sum()), float(usage.sum()), float(out[1].totals.sum())]
                del out
            print(f"{name}: round {rep + 1} of {args.reps}: " + ", ".join(f"{v} {ms[v][-1]:.1f}" for v, _ in runs),
                  file=sys.stderr, flush=True)
        ms.update(split)
        mmm = lambda x: [round(float(np.median(x)), 3), min(x), max(x)]  # noqa: E731
        print(json.dumps({
            "workload": name, "reads": R, "n_nodes": N, "bases": tb, "list_entries": te, "row_entries": rows,
            "usage_row_entries": usage_rows, "keys_per_base": round(rows / max(tb, 1), 3),
            "bytes_off_device": {"parent": 24 * te + 8 * R, "usage_handle": 24 * N + 8 * R, "pileup_handle": 72 * N + 8 * R,
                                 "pileup_export": 72 * N + 8 * R + 36 * rows + 8 * (R + 1)},
            "ms": ms,
            "median_min_max": {v: mmm(x) for v, x in ms.items()},
            "device_ms_index2_median_min_max": {v: mmm(x) for v, x in dev.items()},
            "launches_index2": launches,
            "ranges_of_parent_and_pileup_handle_overlap": not (max(ms["pileup_handle"]) < min(ms["parent"])
                                                               or max(ms["parent"]) < min(ms["pileup_handle"])),
            "checksums (row entries, sum of keys, sum of usage, sum of totals)": sums}), flush=True)
        # the next workload's adaptive pass plans with all the memory the device has: give this one's back first
        del gm, rc, mp
        L.phmm_release_workspace()


if __name__ == "__main__":
    main()
