"""Time the greedy search of sample_posterior (multi_dbg/posterior.rs:314-417) on cfg3, two ways:

  side A  the parent commit's library, driving the loop the only way it can: one
          phmm_full_prob_reads_copy_num_changes call per iteration with the host applying the move to its own vector;
  side B  this commit's device-side state (phmm_likelihood): score_changes + move per iteration.

A search is `--iters` iterations from the graph's own copy numbers; each iteration scores C candidates given as changes
to the current vector and moves to one of them (fixed seed: both sides walk the same sequence).  Shapes as in
tools/copy_num_changes_time.py: `bench` (16 random k-mers +-1 per candidate) and `bubble` (bubble swaps).  Only totals
are asked for (out_logp = NULL), as the sampler does.

Each side runs in a fresh child process of its own that imports ITS tree (`--parent-root`: a checkout of the parent
commit with its library built; side B: this tree), builds the workload once and then serves search requests over a
pipe, so that the two sides alternate on one box: per cell one warm-up search each, then `--reps` rounds A, B, A, B ...
timed with a host clock around the synchronous calls.  Prints one JSON line per cell: ms per iteration of both sides
(median, min, max over the repetitions), side A's spread, and the largest per-read difference between the two sides
after the last iteration.

    python tools/likelihood_time.py --parent-root DIR [--cands 64,256,1024] [--shapes bench,bubble] [--reps 5]
    python tools/likelihood_time.py --serve A|B --root DIR        (the children)

The split of a call into its sections (base pass, host loops, mask kernels, scoring classes, compose) is a run of its
own, because the trace synchronises the stream at every section: a child on this tree under PHMM_TRACE=1, requests on
its standard input, the sections on its standard error --
    echo '{"shape": "bubble", "C": 64, "iters": 6}' | PHMM_TRACE=1 python tools/likelihood_time.py --serve A --root .
(side A on this tree is the stateless call with the trace points; --serve B is the handle).  The kernel tables are the
same children under `rocprofv3 --kernel-trace --stats`.  profiles/likelihood_session.txt holds all three.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def candidates(shape, vec, swaps, Cn, it):
    """C candidates as changes to `vec` -> [(nodes, new cns)]; the same for both sides (seeded by the iteration)"""
    rng = np.random.default_rng(1000 + it)
    out = []
    for c in range(Cn):
        if shape == "bench":
            ix = np.unique(rng.integers(0, vec.size, size=16))
            out.append((ix, np.maximum(vec[ix].astype(np.int64) + rng.choice([-1, 1], size=ix.size), 0)))
        else:
            a_only, b_only = swaps[(it * 7 + c) % len(swaps)]
            out.append((np.concatenate([a_only, b_only]),
                        np.concatenate([vec[a_only].astype(np.int64) + 1,
                                        np.maximum(vec[b_only].astype(np.int64) - 1, 0)])))
    return out


def csr(cands):
    off = np.zeros(len(cands) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(n) for n, _ in cands])
    node = np.concatenate([np.asarray(n, np.uint32) for n, _ in cands] + [np.zeros(0, np.uint32)])
    cn = np.concatenate([np.asarray(v, np.uint32) for _, v in cands] + [np.zeros(0, np.uint32)])
    return off, node, cn


def serve(side, root):
    """child: imports the tree at `root`, answers {"shape", "C", "iters", "final"} requests line by line"""
    sys.path.insert(0, root)
    import bench  # noqa: E402  (workload builders only)
    import dbgphmm_amd as D  # noqa: E402
    from dbgphmm_amd import _ffi  # noqa: E402
    assert os.path.dirname(os.path.abspath(D.__file__)).startswith(os.path.abspath(root))
    arrays, reads, w = bench.build_workload("cfg3")
    sg, occ = D.dbg_from_haplotypes(bench.cfg_haplotypes("cfg3"), w["k"], with_occurrences=True)
    model = D.PHMMModel(arrays)
    rc = D.ReadCollection(reads)
    mp, _ = model.generate_mappings(rc, None, True)
    base = sg.copy_num.astype(np.uint32)
    swaps = bubbles(sg, occ)
    L = _ffi.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    print(json.dumps(dict(ready=side, reads=len(reads), n_nodes=int(base.size), lib=_ffi.LIB_PATH)), flush=True)
    for line in sys.stdin:
        req = json.loads(line)
        shape, Cn, iters = req["shape"], req["C"], req["iters"]
        pick = np.random.default_rng(7).integers(0, Cn, size=iters)
        vec = base.copy()
        tot, nres = np.empty(Cn), np.empty(Cn, np.uint64)
        ms, rescored, create_ms = 0.0, 0, 0.0
        if side == "B":
            t0 = time.perf_counter()
            lk = model.likelihood(rc, mp, vec, 0)
            create_ms = (time.perf_counter() - t0) * 1e3
        for it in range(iters):
            cands = candidates(shape, vec, swaps, Cn, it)
            off, node, cn = csr(cands)
            nodes, vals = cands[pick[it]]
            nodes, vals = np.asarray(nodes, np.uint32), np.asarray(vals, np.uint32)
            t0 = time.perf_counter()
            if side == "A":
                _ffi.check(L.phmm_full_prob_reads_copy_num_changes(model._h, rc._h, mp._h, p(vec), 0, Cn, p(off), p(node),
                                                                   p(cn), None, p(tot), p(nres)))
                vec[nodes] = vals  # the host applies the move; the next call starts from nothing
            else:
                _ffi.check(L.phmm_likelihood_score_changes(lk._h, Cn, p(off), p(node), p(cn), None, p(tot), p(nres)))
                lk.move(nodes, vals)
                vec[nodes] = vals
            ms += (time.perf_counter() - t0) * 1e3
            rescored += int(nres.sum())
        if side == "A":  # per-read values under the final vector: the base of one more call, with the empty candidate
            _, lp, _ = model.to_full_prob_reads_copy_num_changes(rc, mp, vec, csr([([], [])]), 0)
            final = lp[0]
        else:
            cur_cn, final, _ = lk.current()
            assert np.array_equal(cur_cn, vec)
        if req.get("final"):
            np.save(req["final"], final)
        print(json.dumps(dict(ms_per_iter=ms / iters, create_ms=create_ms,
                              rescored_share=rescored / (iters * Cn * len(reads)), last_total=float(tot[pick[-1]]))),
              flush=True)


class Child:
    def __init__(self, side, root):
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--serve", side, "--root", root],
                                  stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, bufsize=1)
        self.info = self.ask(None)

    def ask(self, req):
        if req is not None:
            self.p.stdin.write(json.dumps(req) + "\n")
            self.p.stdin.flush()
        line = self.p.stdout.readline()
        if not line:
            raise RuntimeError("child ended: exit status %s" % self.p.wait())
        return json.loads(line)

    def close(self):
        self.p.stdin.close()
        return self.p.wait()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--serve", choices=["A", "B"])
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--parent-root")
    ap.add_argument("--cands", default="64,256,1024")
    ap.add_argument("--shapes", default="bench,bubble")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out-dir", help="where the two sides leave their final per-read values (default: a temporary directory)")
    args = ap.parse_args()
    if args.serve:
        return serve(args.serve, args.root)
    if not args.parent_root:
        ap.error("--parent-root: a checkout of the parent commit with its library built")
    tmp = None
    if not args.out_dir:
        tmp = tempfile.TemporaryDirectory()
        args.out_dir = tmp.name
    a = Child("A", os.path.abspath(args.parent_root))
    b = Child("B", HERE)  # (a child that fails ends the run: nothing more is started)
    print(json.dumps(dict(side_a=a.info, side_b=b.info)), flush=True)
    fa, fb = os.path.join(args.out_dir, "final_a.npy"), os.path.join(args.out_dir, "final_b.npy")
    for shape in args.shapes.split(","):
        for Cn in (int(x) for x in args.cands.split(",")):
            req = dict(shape=shape, C=Cn, iters=args.iters)
            a.ask(req)
            b.ask(req)  # warm-up: one search each
            ta, tb, rb = [], [], None
            for _ in range(args.reps):
                ta.append(a.ask(dict(req, final=fa))["ms_per_iter"])
                rb = b.ask(dict(req, final=fb))
                tb.append(rb["ms_per_iter"])
            va, vb = np.load(fa), np.load(fb)
            with np.errstate(invalid="ignore"):
                d = np.where(np.isneginf(va) & np.isneginf(vb), 0.0, np.abs(va - vb))
            print(json.dumps(dict(workload="cfg3", shape=shape, candidates=Cn, iters=args.iters, reps=args.reps,
                                  a_ms_per_iter_median=float(np.median(ta)), a_min=float(np.min(ta)),
                                  a_max=float(np.max(ta)), a_spread=float(np.max(ta) - np.min(ta)),
                                  b_ms_per_iter_median=float(np.median(tb)), b_min=float(np.min(tb)),
                                  b_max=float(np.max(tb)), b_create_ms=rb["create_ms"],
                                  speedup_median=float(np.median(ta) / np.median(tb)),
                                  b_not_above_a_plus_spread=bool(np.median(tb) <= np.median(ta) + np.max(ta) - np.min(ta)),
                                  rescored_share=rb["rescored_share"],
                                  max_abs_delta_final=float(np.max(d)))), flush=True)
    if a.close() or b.close():
        sys.exit(1)


if __name__ == "__main__":
    main()
