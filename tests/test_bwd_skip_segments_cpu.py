"""Segment masks of the dense head's backward kernel ("Run skipping"), the parts that need no GPU.

1. seg_size, segs_per_run_log2 and seg_hull (dbgphmm_amd/csrc/seg_hull.h), which bwd_step shares with the host, compiled into
   a stand-alone program with the host address and undefined-behaviour sanitizers, against a restatement in Python:
   every 8-bit mask, run lengths with 8 segments and with one, full runs and ragged last runs.
2. The property the hull walk rests on, with the oracle's backward tables on the toy graphs of
   tests/golden/toy_dbgs.json: the marks propagated per segment by the kernel's rule from the hand-over column cover
   every node at which a dense backward column is non-zero, so a cell that a row walks inside its hull but outside
   the marks is an exact zero."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import dbgphmm_amd as D
from test_bwd_skip_runs_cpu import _toy_model, descendants, run_successors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dbgphmm_amd", "csrc")
SEGS_PER_RUN = 8
NPTS = [2, 8, 12, 16, 24, 64]

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "seg_hull.h"
// per argument npt: "S <npt> <S> <log2 of the segments per run>", then for every top row jtop of a (ragged) run and
// every mask, with the bits of segments that start above jtop cleared as bwd_step never sets them:
// "<npt> <jtop> <mask> <walks> <first> <top>"
int main(int argc, char **argv) {
    for (int i = 1; i < argc; i++) {
        const int npt = atoi(argv[i]), S = phmm::seg_size(npt);
        printf("S %d %d %d\n", npt, S, phmm::segs_per_run_log2(npt));
        for (int jtop = 0; jtop < npt; jtop++) {
            const int nseg = jtop / S + 1;
            for (unsigned mask = 0; mask < 256; mask++) {
                const unsigned mk = mask & ((1u << nseg) - 1u);
                int first = -1, top = -1;
                const bool walks = phmm::seg_hull(mk, S, jtop, &first, &top);
                printf("%d %d %u %d %d %d\n", npt, jtop, mask, walks ? 1 : 0, first, top);
            }
        }
    }
    return 0;
}
"""


def seg_size(npt):
    return npt // SEGS_PER_RUN if npt % SEGS_PER_RUN == 0 else npt


def hull(mask, S, jtop):
    """the restatement: the nodes of the marked segments up to jtop, and everything between the lowest and the highest"""
    marked = [j for j in range(jtop + 1) if (mask >> (j // S)) & 1]
    if not marked:
        return None
    return min(marked), max(marked) - min(marked)


@pytest.fixture(scope="module")
def hull_table(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    cmd = [cxx] if cxx else ["/opt/rocm/bin/hipcc", "-x", "c++"]
    d = tmp_path_factory.mktemp("seg_hull")
    src, exe = d / "main.cpp", d / "seg_hull_main"
    src.write_text(MAIN)
    subprocess.check_call(cmd + ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                 "-I", CSRC, str(src), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    out = subprocess.run([str(exe)] + [str(n) for n in NPTS], check=True, capture_output=True, text=True, env=env).stdout
    sizes, rows = {}, {}
    for line in out.splitlines():
        t = line.split()
        if t[0] == "S":
            sizes[int(t[1])] = int(t[2])
            assert int(t[1]) == int(t[2]) << int(t[3])  # a run is 8 segments or one
        else:
            npt, jtop, mask, walks, first, top = map(int, t)
            rows[npt, jtop, mask] = (walks, first, top)
    return sizes, rows


def test_segment_size(hull_table):
    sizes, _ = hull_table
    assert sizes == {npt: seg_size(npt) for npt in NPTS}
    assert sizes == {2: 2, 8: 1, 12: 12, 16: 2, 24: 3, 64: 8}


@pytest.mark.parametrize("npt", NPTS)
def test_hull_bounds_match_restatement(hull_table, npt):
    _, rows = hull_table
    S = seg_size(npt)
    n = 0
    for jtop in range(npt):  # npt - 1: a full run; below: the ragged last run of a column
        valid = (1 << (jtop // S + 1)) - 1
        for mask in range(256):
            walks, first, top = rows[npt, jtop, mask]
            want = hull(mask & valid, S, jtop)
            if want is None:
                assert walks == 0, (npt, jtop, mask)
                continue
            assert walks == 1 and (first, top) == want, (npt, jtop, mask, first, top, want)
            assert first % S == 0 and 0 <= top and first + top <= jtop
            n += 1
    assert n > 0
    if S == npt:
        # one segment per run: a marked run is walked in full, as before the segments
        assert all(rows[npt, jtop, m] == (1, 0, jtop) for jtop in range(npt) for m in range(1, 256, 2))


@pytest.mark.parametrize("name", ["circular", "linear", "intersection", "selfloop", "repeat"])
def test_segment_marks_cover_the_oracle_support(oracle, name):
    """One read per group (the tightest mask), runs of 8 segments of S = 1, 2, 3 nodes.  H = the segments of the
    hand-over column (the first sparse backward table behind the dense head); a segment is marked in column pos if it
    is in H, was marked one column later, or has a segment successor of which either holds.  Every node with a non-zero
    m or i lies in a marked segment, and every cell inside the hull of a run's marks but outside them is zero."""
    checked = switched = inside = 0
    for n_warmup in (2, 4):
        arrays = _toy_model(name, n_warmup)
        n = arrays.n_nodes
        om = oracle.Model(arrays)
        live = np.isfinite(arrays.trans_logp)
        edges = list(zip(arrays.edge_src[live].tolist(), arrays.edge_dst[live].tolist()))
        desc = descendants(n, edges, int(arrays.param.n_max_gaps) + 2)
        reads = D.sample_reads(arrays, 10 ** 9, 14, seed=3, max_reads=12)
        for S in (1, 2, 3):
            ss = run_successors(n, S, desc)
            nseg = len(ss)
            seg_of = np.arange(n) // S
            run_of = seg_of // SEGS_PER_RUN
            for read in reads:
                for umr in (True, False):
                    b = om.run_sparse_adaptive(read, umr).backward
                    dense = [i for i in range(len(read)) if b.is_dense(i)]
                    if not dense:
                        continue
                    s0 = max(dense)
                    assert dense == list(range(s0 + 1))
                    if s0 == len(read) - 1:
                        continue  # a `first` lane: every segment is marked from its last column on
                    switched += 1
                    m, i, _, _ = b.table(s0 + 1)
                    H = np.zeros(nseg, bool)
                    H[np.flatnonzero((m > -np.inf) | (i > -np.inf)) // S] = True
                    A = np.zeros(nseg, bool)
                    for pos in range(s0, -1, -1):
                        on = H | A
                        A = np.array([on[sg] or any(on[t] for t in ss[sg]) for sg in range(nseg)])
                        assert (A | ~on).all()  # marks only grow towards column 0
                        m, i, _, _ = b.table(pos)
                        nz = (m > -np.inf) | (i > -np.inf)
                        assert A[seg_of[nz]].all(), (name, n_warmup, S, pos, np.flatnonzero(nz).tolist(), np.flatnonzero(A).tolist())
                        checked += int(nz.sum())
                        # the hull of each run's marks: what its row walks
                        for rho in np.unique(run_of[A[seg_of]]):
                            sg = np.flatnonzero(A & (np.arange(nseg) // SEGS_PER_RUN == rho))
                            walked = (seg_of >= sg.min()) & (seg_of <= sg.max())
                            extra = walked & ~A[seg_of]
                            assert not nz[extra].any(), (name, n_warmup, S, pos, int(rho))
                            inside += int(extra.sum())
    print(f"\n{name}: reads with a sparse tail {switched}, non-zero cells checked {checked}, "
          f"unmarked cells inside a hull {inside}")
    assert switched > 0 and checked > 0
