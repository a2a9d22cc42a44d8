"""Time the weighted walk and the maximum-expected-accuracy path over mapping lists (include/phmm_amd_mea.h) against the
two calls they are made of, in ONE process:

  weighted_path    run_with_mapping_weighted_path, weights in device memory, out_path = NULL (score and counts only)
  mea_path         run_with_mapping_mea_path, out_path in host memory, no weights copied out
  mea_path_null    the same with out_path = NULL
  best_path_null   run_with_mapping_best_path with out_path = NULL: the same recursion without the 24-byte read per entry
  states_best      run_with_mapping_states with out_state_logp = NULL: the states half of the MEA call without values

    python tools/mea_path_time.py [--workloads rep20,cfg3] [--reps 7] [--warmup 2] [--drawn 256]

cfg3 and rep20 are bench.py's workloads; the lists are those of a generate_mappings(None) call.  After `--warmup` calls of
everything the calls take turns `--reps` times, no knob set.  Expected, not asserted: weighted_path about best_path_null
(one more 24-byte read per entry), mea_path_null about states_best plus weighted_path.  Prints one JSON line per workload:
wall ms of each repetition (host clock around the synchronous call), median, minimum and maximum, the two ratios, and a
figure of merit on `--drawn` reads drawn from the workload's model with PHMMModel.sample_reads(want_history=True): the
share of bases whose true node (the node of the state that emitted the base; InsBegin has none) is the node of the MEA
path, of the best path, and of the per-base decoding of the states call.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

NO_NODE = -1


def true_nodes(history):
    """node of the emitting state of every base of one drawn read (NO_NODE for InsBegin)"""
    out = []
    for wd in history.tolist():
        if wd == 0xFFFFFFFD:
            out.append(NO_NODE)
        elif wd < 0xFFFFFFFC and wd & 3 != 2:
            out.append(wd >> 2)
    return np.array(out, dtype=np.int64)


def code_nodes(codes, po, nd):
    """node of one (slot << 2) | kind code per base (NO_NODE for InsBegin and for no code)"""
    codes = codes.astype(np.int64)
    ok = codes < 0xFFFFFFFC
    idx = np.where(ok, po[:-1].astype(np.int64) + (codes >> 2), 0)
    return np.where(ok, nd[np.minimum(idx, max(len(nd) - 1, 0))].astype(np.int64), NO_NODE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="rep20,cfg3")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--drawn", type=int, default=256)
    args = ap.parse_args()
    import bench
    import dbgphmm_amd as D
    from dbgphmm_amd import _ffi, _ffi_mea
    L = _ffi_mea.lib()
    _ffi.check(L.phmm_set_device(0))
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes, hip.hipMemcpy.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], [C.c_void_p]

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        return (time.perf_counter() - t0) * 1e3, out

    for name in args.workloads.split(","):
        arrays, reads, _ = bench.build_workload(name)
        gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
        mp, _ = gm.generate_mappings(rc, None, True)
        R, te = len(reads), int(L.phmm_mappings_total_entries(mp._h))
        # the MEA weights of this workload, once, as the device weights of the weighted walk
        w = gm.run_with_mapping_mea_path(rc, mp, want_path=False, want_weights=True)[4]
        d_w = C.c_void_p()
        assert hip.hipMalloc(C.byref(d_w), w.nbytes) == 0 and hip.hipMemcpy(d_w, w.ctypes.data_as(C.c_void_p), w.nbytes, 1) == 0
        score, counts = np.empty(R), np.empty((R, 4), dtype=np.uint32)
        P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

        def weighted_path():
            _ffi.check(L.phmm_run_with_mapping_weighted_path(gm._h, rc._h, mp._h, d_w, None, P(score), None, P(counts)))
            return [float(score.sum()), int(counts.astype(np.int64).sum())]

        def mea_path():
            lf, s, path, c, _ = gm.run_with_mapping_mea_path(rc, mp)
            return [float(s.sum()), int(c.astype(np.int64).sum()), int((path[:, 1:] != D.PATH_NONE).sum())]

        def mea_path_null():
            lf, s, _, c, _ = gm.run_with_mapping_mea_path(rc, mp, want_path=False)
            return [float(s.sum()), int(c.astype(np.int64).sum())]

        def best_path_null():
            lp, _, c = gm.run_with_mapping_best_path(rc, mp, want_path=False)
            return [float(lp.sum()), int(c.astype(np.int64).sum())]

        def states_best():
            lf, _, best = gm.run_with_mapping_states(rc, mp, want_states=False)
            return [float(lf.sum()), int(best.astype(np.uint64).sum())]

        runs = [("weighted_path", weighted_path), ("mea_path", mea_path), ("mea_path_null", mea_path_null),
                ("best_path_null", best_path_null), ("states_best", states_best)]
        for _ in range(args.warmup):
            for _, fn in runs:
                timed(fn)
        ms = {v: [] for v, _ in runs}
        sums = {}
        for _ in range(args.reps):
            for v, fn in runs:
                t, out = timed(fn)
                ms[v].append(round(t, 3))
                sums[v] = out
        med = {v: float(np.median(x)) for v, x in ms.items()}
        hip.hipFree(d_w)

        # the figure of merit: reads drawn from the model, their true states known
        length = int(np.median([len(r) for r in reads]))
        drc, info = gm.sample_reads(length, "state_count", n_reads=args.drawn, seed=1, want_history=True)
        dmp, _ = gm.generate_mappings(drc, None, True)
        po, nd, _ = dmp.arrays()
        truth = np.concatenate([true_nodes(h) for h in info["history"]])
        assert truth.size == drc.total_bases()
        mea = gm.run_with_mapping_mea_path(drc, dmp)[2][:, 0]
        bp = gm.run_with_mapping_best_path(drc, dmp)[1][:, 0]
        dec = gm.run_with_mapping_states(drc, dmp, want_states=False)[2]
        share = {k: round(float((code_nodes(c, po, nd) == truth).mean()), 5) for k, c in (("mea_path", mea), ("best_path", bp), ("states_decoding", dec))}
        print(json.dumps({
            "workload": name, "reads": R, "n_nodes": int(arrays.n_nodes), "bases": int(rc.total_bases()), "list_entries": te,
            "ms": ms, "median_min_max": {v: [round(med[v], 3), min(x), max(x)] for v, x in ms.items()},
            "weighted_path_over_best_path_null": round(med["weighted_path"] / med["best_path_null"], 3),
            "mea_path_null_over_states_best_plus_weighted_path": round(med["mea_path_null"] / (med["states_best"] + med["weighted_path"]), 3),
            "checksums": sums,
            "drawn": {"reads": len(drc), "length": length, "bases": int(truth.size), "true_node_share": share}}), flush=True)
        del gm, rc, mp, drc, dmp
        L.phmm_release_workspace()


if __name__ == "__main__":
    main()
