"""Run skipping of the dense head's backward kernel (bwd_step<64>, DESIGN.md section 6, "Run skipping"): generate_mappings with the
run masks and with PHMM_NO_BWD_SKIP=1 (every run computed, the kernel as it was) in one process give the same bits --
mapping lists, node usage, forward and backward ln P per read -- under the knobs that change what reads the
emit-prob planes, on graphs with branches, cycles and hubs, and with reads that end inside the dense head next to reads
with a sparse tail.  One case is held to the oracle as well, and one shows that runs are skipped at all."""
import numpy as np
import pytest

import dbgphmm_amd as D
from dbgphmm_amd import _ffi
from fuzz_cases import make_case
from graph_cases import base_case
from helpers import scores_tie_aware, small_dbg_model
from repeat_cases import dataset

pytestmark = pytest.mark.gpu

STATS_DENSE_BWD = 1


def _mix_lengths(reads, n_warmup):
    """Reads cut to 1, 2, n_warmup - 1 and n_warmup + 3 bases among the others (`first` lanes and sparse-tail lanes in
    one group), at most 200 reads of at most 200 bases, and not a multiple of 64 of them (empty lanes)."""
    reads = [bytes(r[:200]) for r in reads[:198]]
    for j, n in enumerate((1, 2, max(1, n_warmup - 1), n_warmup + 3)):
        src = reads[(5 * j + 1) % len(reads)]
        reads.insert((7 * j + 2) % len(reads), src[:n])
    if len(reads) % 64 == 0:
        reads.append(reads[0][: n_warmup + 3])
    return reads


def _run(arrays, reads, umr, monkeypatch, env, skip):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if skip:
        monkeypatch.delenv("PHMM_NO_BWD_SKIP", raising=False)
    else:
        monkeypatch.setenv("PHMM_NO_BWD_SKIP", "1")
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    mp, nf = gm.generate_mappings(rc, None, umr)
    cells = _ffi.last_call_stats(STATS_DENSE_BWD)[2]
    cols, flags = (x.copy() for x in rc.last_call_info()) if umr else (None, None)
    return dict(cols=cols,arrays=[x.copy() for x in mp.arrays()], nf=nf.copy(), lf=mp.read_logp()[1].copy(),
                lb=mp.read_logp_backward()[1].copy(), cells=cells, flags=flags)


def _same(a, b):
    for x, y in zip(a["arrays"], b["arrays"]):
        assert np.array_equal(x, y)
    assert np.array_equal(a["nf"], b["nf"])
    assert np.array_equal(a["lf"], b["lf"])
    assert np.array_equal(a["lb"], b["lb"])


def _pair(arrays, reads, umr, monkeypatch, npt, env=None, skipped=False):
    """skipped: the read set has sparse-tail reads on a graph of many runs, so the masked call must have walked fewer
    cells than the other one -- the masks really reached the kernel under this environment"""
    env = dict({"PHMM_DENSE_W": "64", "PHMM_DENSE_NPT": str(npt)}, **(env or {}))
    on = _run(arrays, reads, umr, monkeypatch, env, True)
    off = _run(arrays, reads, umr, monkeypatch, env, False)
    _same(on, off)
    print(f"\ncells: skip {on['cells']}, no skip {off['cells']}")
    assert on["cells"] <= off["cells"]
    if skipped:
        assert 0 < on["cells"] < off["cells"]
    return on, off


@pytest.fixture(scope="module")
def dbg900():
    arrays, sg = small_dbg_model(900, 16, 0.003, seed=21, min_copy_num=1)
    reads = D.sample_reads(arrays, 10 ** 9, 150, seed=5, max_reads=190)
    reads = [r[: max(1, len(r) - (j * 13) % 149)] for j, r in enumerate(reads)]
    return arrays, _mix_lengths(reads, arrays.param.n_warmup)


@pytest.mark.parametrize("case", [0, 1, 2, 3])
@pytest.mark.parametrize("umr", [True, False])
def test_fuzz_cases(gpu_lib, monkeypatch, case, umr):
    c = make_case(np.random.default_rng(20261018 + case), case)
    reads = _mix_lengths(list(c["reads"]), c["arrays"].param.n_warmup)
    _pair(c["arrays"], reads, umr, monkeypatch, 2 if case % 2 else 8)


@pytest.mark.parametrize("graph", ["zoo", "zoo_lean", "dbg"])
@pytest.mark.parametrize("npt", [2, 8])
def test_graphs_that_are_not_dbgs(gpu_lib, monkeypatch, graph, npt):
    """the zoo graph: self-loop, parallel edge, a hub of 7 arms, a back edge 30 nodes upstream, no chain flags"""
    b = base_case(graph)
    reads = _mix_lengths(list(b["reads"]), b["arrays"].param.n_warmup)
    for umr in (True, False):
        _pair(b["arrays"], reads, umr, monkeypatch, npt)


@pytest.mark.parametrize("npt", [2, 8])
def test_tandem_repeat(gpu_lib, monkeypatch, npt):
    arrays, reads, sg, haps = dataset("u20", 40, read_len=200, max_reads=150)
    _pair(arrays, _mix_lengths(list(reads), arrays.param.n_warmup), True, monkeypatch, npt)


@pytest.mark.parametrize("env", [
    {},
    {"PHMM_NO_RUNMAX": "1"},
    {"PHMM_FORCE_RADIX": "1"},
    {"PHMM_BWD_DMA": "1"},
    {"PHMM_WARM_COLS": "4", "PHMM_NO_KEEP_ALL": "1"},  # reads still dense at column 4 go to the side plan
    {"PHMM_WARM_COLS": "4"},
    {"PHMM_WORKERS": "3", "PHMM_CHUNK_GROUPS": "1", "PHMM_PIPELINE_MIN_GROUPS": "2"},
], ids=lambda e: "+".join(sorted(e)) or "default")
@pytest.mark.parametrize("npt", [2, 8])
def test_knobs(gpu_lib, monkeypatch, dbg900, env, npt):
    arrays, reads = dbg900
    for umr in (True, False):
        # (PHMM_NO_KEEP_ALL defers every read with a sparse tail to the side plan, whose launches the statistics leave
        # out: the main plan keeps the reads that end inside its four columns, and those compute every run)
        _pair(arrays, reads, umr, monkeypatch, npt, env, skipped="PHMM_NO_KEEP_ALL" not in env)


def test_against_the_oracle(gpu_lib, oracle, monkeypatch, dbg900):
    """the pair is not merely equal to each other: backward totals against run_sparse_adaptive (tie-aware, 1e-6)"""
    arrays, reads = dbg900
    on, off = _pair(arrays, reads, True, monkeypatch, 8, skipped=True)
    om = oracle.Model(arrays)
    keep = [i for i in range(0, len(reads), 4) if not on["flags"][i] & _ffi.PHMM_READ_FORCED_SWITCH]
    keep += [i for i, r in enumerate(reads) if len(r) <= arrays.param.n_warmup + 3 and i not in keep]

    def want(i):
        return om.run_sparse_adaptive(reads[i], True).to_full_prob_backward()
    scores_tie_aware(oracle, on["lb"][keep], np.array([want(i) for i in keep]), lambda b: want(keep[b]))
    assert len(keep) >= 40


def test_runs_are_skipped(gpu_lib, monkeypatch):
    """The first 64 reads of cfg1m, W = 64, runs of 8 nodes.  The oracle's share of runs that hold a non-zero value for
    one of these reads is 0.42; the kernel activates a whole run per column where the true reach is 6 nodes, hence the
    margin.  Measured on an MI355X: cells(skip) / cells(no skip) = 3 240 824 / 4 809 024 = 0.674, which is also what
    the kernel's rule gives when it is replayed on the oracle's tables of these reads (0.52 of the cells lie in a run
    with a non-zero value there)."""
    import bench
    arrays, reads, w = bench.build_workload("cfg1m", 0)
    reads = reads[:64]
    on, off = _pair(arrays, reads, True, monkeypatch, 8)
    # the dense count: every node of every dense backward column of every read -- columns 0 .. switch position for a
    # read with a sparse tail, the whole read otherwise (no read of this set is deferred to the side plan, whose
    # launches the statistics leave out)
    assert not np.any(on["flags"] & _ffi.PHMM_READ_DEFERRED)
    lens = np.array([len(r) for r in reads], dtype=np.int64)
    cols = on["cols"].astype(np.int64)
    dense = int(np.where(cols < lens, cols + 1, lens).sum()) * arrays.n_nodes
    print(f"\ncells: skip {on['cells']}, no skip {off['cells']}, dense count {dense}, share {on['cells'] / off['cells']:.3f}")
    assert off["cells"] == dense
    assert on["cells"] < 0.8 * off["cells"]
