"""Time the tables over mapping lists (phmm_run_with_mapping_tables) against the states call, on the same lists, in ONE
process:

  forward   the forward half alone, all three of its outputs into host buffers
  backward  the backward half alone, all three of its outputs into host buffers
  device    both halves, every output into device buffers (nothing is staged, nothing leaves the device)
  host      both halves, every output into host buffers (48 bytes per list entry + 32 per base leave the device)
  states    phmm_run_with_mapping_states with its values (24 bytes per list entry + 4 per base)

    python tools/list_tables_time.py [--workloads rep20,cfg3] [--reps 7] [--warmup 2]

cfg3 and rep20 are bench.py's workloads; the lists are those of a generate_mappings(None) call.  After `--warmup` calls of
everything (workspace growth, code objects) the calls take turns `--reps` times with no knob set.  Prints one JSON line per
workload: wall ms of each repetition (host clock around the synchronous call), median, minimum and maximum,
phmm_last_call_stats(2) of the last call of each variant, and checksums (sums of the finite values, taken outside the
timed region) that show the variants computed the same thing.
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


class _DeviceDoubles:
    """n doubles of device memory from the HIP runtime the library is linked against"""

    def __init__(self, n):
        self.hip, self.n, self.p = C.CDLL("libamdhip64.so"), int(n), C.c_void_p()
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipFree.argtypes = [C.c_void_p]
        assert self.hip.hipMalloc(C.byref(self.p), max(8 * self.n, 1)) == 0

    def numpy(self):
        out = np.empty(self.n)
        if self.n:
            assert self.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), self.p, 8 * self.n, 2) == 0  # device to host
        return out

    def free(self):
        if self.p:
            self.hip.hipFree(self.p)
            self.p = C.c_void_p()


def _finite_sum(a):
    a = np.asarray(a)
    return float(a[np.isfinite(a)].sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="rep20,cfg3")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import bench
    import dbgphmm_amd as D
    from dbgphmm_amd import _ffi, _ffi_tables
    L = _ffi.lib()
    TL = _ffi_tables.lib()
    _ffi.check(L.phmm_set_device(0))
    L.phmm_enable_timing(1)

    for name in args.workloads.split(","):
        arrays, reads, _ = bench.build_workload(name)
        gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
        mp, _ = gm.generate_mappings(rc, None, True)
        po = mp.arrays()[0].astype(np.int64)
        off = rc.offsets.astype(np.int64)
        rmax = np.array([np.diff(po[off[r]:off[r + 1] + 1]).max(initial=0) for r in range(len(reads))])
        R, te, tb = len(reads), int(po[-1]), int(off[-1])
        dev = [_DeviceDoubles(n) for n in (R, R, 3 * te, 2 * tb, 3 * te, 2 * tb)]

        # each variant returns what the call returned; the checksums are taken outside the timed region
        def forward():
            return gm.run_with_mapping_tables(rc, mp, want_backward=False)

        def backward():
            return gm.run_with_mapping_tables(rc, mp, want_forward=False)

        def host():
            return gm.run_with_mapping_tables(rc, mp)

        def device():
            _ffi.check(TL.phmm_run_with_mapping_tables(gm._h, rc._h, mp._h, *[d.p for d in dev]))
            return None

        def states():
            return gm.run_with_mapping_states(rc, mp)

        def checksums(v, out):
            if v == "states":
                lf, sl, best = out
                return [float(lf.sum()), float(np.exp(sl).sum()), int(best.astype(np.uint64).sum())]
            if v == "device":
                h = [d.numpy() for d in dev]
                lf, lb, f, fs, b, bs = h
            else:
                lf, lb, f, fs, b, bs = out.logp_forward, out.logp_backward, out.fwd, out.fwd_scal, out.bwd, out.bwd_scal
            return [None if a is None else _finite_sum(a) for a in (lf, f, fs, lb, b, bs)]

        runs = [("forward", forward), ("backward", backward), ("device", device), ("host", host), ("states", states)]

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
        last = {}
        for rep in range(args.reps):
            for v, fn in runs:
                t, out, st = timed(fn)
                ms[v].append(round(t, 3))
                last[v] = {"stats2": st}
                if rep + 1 == args.reps:
                    last[v]["checksums"] = checksums(v, out)
                del out
        print(json.dumps({
            "workload": name, "reads": R, "n_nodes": int(arrays.n_nodes), "bases": tb, "list_entries": te,
            "read_max_list": {"min": int(rmax.min()), "median": float(np.median(rmax)), "max": int(rmax.max()),
                              "at_most_64": int((rmax <= 64).sum()), "65_400": int(((rmax > 64) & (rmax <= 400)).sum())},
            "ms": ms,
            "median_min_max": {v: [round(float(np.median(x)), 3), min(x), max(x)] for v, x in ms.items()},
            "last": last}), flush=True)
        # the next workload's adaptive pass plans with all the memory the device has: give this one's back first
        for d in dev:
            d.free()
        del gm, rc, mp, dev
        L.phmm_release_workspace()


if __name__ == "__main__":
    main()
