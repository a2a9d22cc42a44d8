"""Run skipping of the dense head's backward kernel ("Run skipping"), the parts that need no GPU.

1. build_run_successors (dbgphmm_amd/csrc/run_succ.h), compiled into a stand-alone program with the host address and
   undefined-behaviour sanitizers, against a restatement in Python on small graphs.
2. The property the change rests on, with the oracle's backward tables on the toy graphs of tests/golden/toy_dbgs.json:
   the run masks propagated by the kernel's rule from the hand-over column cover every node at which a dense backward
   column is non-zero."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import dbgphmm_amd as D
from dbgphmm_amd import formats as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dbgphmm_amd", "csrc")
CHAIN_HOPS = 6

MAIN = r"""
#include <cstdio>
#include "run_succ.h"
// input: N npt n_desc, then N+1 offsets, then the entries; output: nrun, the offsets, the entries
int main(int argc, char **argv) {
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    unsigned N, npt, nd;
    if (fscanf(f, "%u %u %u", &N, &npt, &nd) != 3) return 3;
    std::vector<uint32_t> off(N + 1), ent(nd), rs_off, rs;
    for (auto &x : off) if (fscanf(f, "%u", &x) != 1) return 3;
    for (auto &x : ent) if (fscanf(f, "%u", &x) != 1) return 3;
    fclose(f);
    phmm::build_run_successors(N, npt, off, ent, rs_off, rs);
    printf("%zu\n", rs_off.size() - 1);
    for (auto x : rs_off) printf("%u ", x);
    printf("\n");
    for (auto x : rs) printf("%u ", x);
    printf("\n");
    return 0;
}
"""


def descendants(n, edges, hops):
    """per node: the nodes reached by walks of 1 .. hops edges (a list with repeats, as the hop entries have them)"""
    chi = [[] for _ in range(n)]
    for s, d in edges:
        chi[s].append(d)
    out = []
    for v in range(n):
        seen, front = [], [v]
        for _ in range(hops):
            front = [u for w in front for u in chi[w]]
            front = sorted(set(front))
            seen.extend(front)
        out.append(seen)
    return out


def run_successors(n, npt, desc):
    """the restatement: per run, the sorted other runs that hold a descendant of one of its nodes"""
    nrun = (n + npt - 1) // npt
    rs = [set() for _ in range(nrun)]
    for v in range(n):
        rs[v // npt].update(u // npt for u in desc[v])
    return [sorted(s - {rho}) for rho, s in enumerate(rs)]


def _unitig(n):
    return n, [(v, v + 1) for v in range(n - 1)]


def _bubble():
    # 0..19 -> arms 20..23 (next run at npt = 8 and below) and 60..63 (far away) -> 24..59
    n = 64
    e = [(v, v + 1) for v in range(19)] + [(19, 20), (20, 21), (21, 22), (22, 23), (23, 24)]
    e += [(19, 60), (60, 61), (61, 62), (62, 63), (63, 24)] + [(v, v + 1) for v in range(24, 59)]
    return n, e


def _cycle():
    # a tandem repeat: the unit 10..29 closes on itself, the descendant of 29 sits in a lower run
    n = 45
    return n, [(v, v + 1) for v in range(n - 1)] + [(29, 10)]


def _fan():
    # node 5 has out-degree 4, the arms start in four different places
    n = 70
    e = [(v, v + 1) for v in range(5)] + [(5, 6), (5, 20), (5, 40), (5, 66)]
    e += [(v, v + 1) for v in range(6, 19)] + [(v, v + 1) for v in range(20, 39)] + [(v, v + 1) for v in range(40, 65)]
    e += [(v, v + 1) for v in range(66, 69)]
    return n, e


GRAPHS = {"unitig": _unitig(150), "unitig_ragged": _unitig(67), "tiny": _unitig(5), "bubble": _bubble(),
          "cycle": _cycle(), "fan": _fan()}


@pytest.fixture(scope="module")
def builder(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    cmd = [cxx] if cxx else ["/opt/rocm/bin/hipcc", "-x", "c++"]
    d = tmp_path_factory.mktemp("run_succ")
    src, exe = d / "main.cpp", d / "run_succ_main"
    src.write_text(MAIN)
    subprocess.check_call(cmd + ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                 "-I", CSRC, str(src), "-o", str(exe)])

    def run(n, npt, desc):
        off = np.concatenate([[0], np.cumsum([len(x) for x in desc])]).astype(np.int64)
        inp = d / "in.txt"
        inp.write_text(f"{n} {npt} {off[-1]}\n" + " ".join(map(str, off)) + "\n" + " ".join(str(u) for x in desc for u in x) + "\n")
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
        out = subprocess.run([str(exe), str(inp)], check=True, capture_output=True, text=True, env=env).stdout.split("\n")
        nrun = int(out[0])
        o = [int(x) for x in out[1].split()]
        e = [int(x) for x in out[2].split()]
        assert len(o) == nrun + 1 and o[0] == 0 and o[-1] == len(e)
        return [e[o[r]:o[r + 1]] for r in range(nrun)]
    return run


@pytest.mark.parametrize("name", sorted(GRAPHS))
@pytest.mark.parametrize("npt", [2, 8, 64])
def test_run_successors_match_restatement(builder, name, npt):
    n, edges = GRAPHS[name]
    desc = descendants(n, edges, CHAIN_HOPS)
    got, want = builder(n, npt, desc), run_successors(n, npt, desc)
    assert got == want
    nrun = (n + npt - 1) // npt
    assert len(got) == nrun
    if name.startswith("unitig") or name == "tiny":
        # on a unitig the list is {rho + 1} (npt >= the hops of the closure; shorter runs reach further)
        for rho in range(nrun):
            hi = min(nrun - 1, (min(n - 1, rho * npt + npt - 1 + CHAIN_HOPS)) // npt)
            assert got[rho] == list(range(rho + 1, hi + 1))
            if npt >= CHAIN_HOPS:
                assert got[rho] == ([rho + 1] if rho + 1 < nrun else [])
    if name == "cycle" and npt in (2, 8):
        assert any(t < rho for rho, l in enumerate(got) for t in l)  # the descendant in a lower run
    if name == "bubble" and npt == 8:
        assert 7 in got[2] and 3 in got[7]  # 19 -> 60.., 63 -> 24
    if name == "fan" and npt == 8:
        assert {2, 5, 8} <= set(got[0])


def _toy_model(name, n_warmup):
    toy = json.load(open(os.path.join(ROOT, "tests", "golden", "toy_dbgs.json")))[name]
    kmers = [x.encode() for x in toy["kmers"]]
    sg = F.dbg_from_seq_graph_kmers(kmers, toy["copy_nums"], toy["k"]).to_seq_graph()
    param = D.PHMMParams.uniform(0.01).with_(n_warmup=n_warmup, warmup_threshold=2)
    return D.vectorised_to_phmm(sg, param, 1)


@pytest.mark.parametrize("name", ["circular", "linear", "intersection", "selfloop", "repeat"])
def test_masks_cover_the_oracle_support(oracle, name):
    """One read per group (the tightest mask).  H = the runs of the hand-over column (the first sparse backward table
    behind the dense head), A by the rule of bwd_step: a run is computed if it is in H, was computed one column later,
    or has a run successor of which either holds.  Every node with a non-zero m or i lies in a computed run."""
    checked = switched = 0
    for n_warmup in (2, 4):
        arrays = _toy_model(name, n_warmup)
        n = arrays.n_nodes
        om = oracle.Model(arrays)
        live = np.isfinite(arrays.trans_logp)
        edges = list(zip(arrays.edge_src[live].tolist(), arrays.edge_dst[live].tolist()))
        desc = descendants(n, edges, int(arrays.param.n_max_gaps) + 2)
        reads = D.sample_reads(arrays, 10 ** 9, 14, seed=3, max_reads=12)
        for npt in (1, 2, 3):
            rs = run_successors(n, npt, desc)
            nrun = len(rs)
            for read in reads:
                for umr in (True, False):
                    b = om.run_sparse_adaptive(read, umr).backward
                    dense = [i for i in range(len(read)) if b.is_dense(i)]
                    if not dense:
                        continue
                    s0 = max(dense)
                    assert dense == list(range(s0 + 1))
                    if s0 == len(read) - 1:
                        continue  # a `first` lane: every run is computed from its last column on
                    switched += 1
                    m, i, _, _ = b.table(s0 + 1)
                    H = np.zeros(nrun, bool)
                    H[np.flatnonzero((m > -np.inf) | (i > -np.inf)) // npt] = True
                    A = np.zeros(nrun, bool)
                    for pos in range(s0, -1, -1):
                        on = H | A
                        A = np.array([on[rho] or any(on[t] for t in rs[rho]) for rho in range(nrun)])
                        m, i, _, _ = b.table(pos)
                        nz = np.flatnonzero((m > -np.inf) | (i > -np.inf))
                        assert A[nz // npt].all(), (name, n_warmup, npt, pos, nz.tolist(), np.flatnonzero(A).tolist())
                        checked += nz.size
    print(f"\n{name}: reads with a sparse tail {switched}, non-zero cells checked {checked}")
    assert switched > 0 and checked > 0
