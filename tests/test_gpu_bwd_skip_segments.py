"""Segment masks and the hull walk of the dense head's backward kernel (bwd_step<64>, DESIGN.md section 6, "Run skipping"):
generate_mappings with the masks and with PHMM_NO_BWD_SKIP=1 in one process give the same bits -- mapping lists, node
usage, forward and backward ln P per read -- at run lengths whose segments hold 2, 3 and 8 nodes (npt = 16, 24, 64) and
at one that keeps a single mask per run (npt = 12), on graphs whose node counts are no multiple of the segment (1127,
178 and 555 nodes).  One case is held to the oracle as well, and one shows how much the segments skip."""
import numpy as np
import pytest

from dbgphmm_amd import _ffi
from graph_cases import base_case
from helpers import scores_tie_aware
from repeat_cases import dataset
from test_gpu_bwd_skip import _mix_lengths, _pair, dbg900  # noqa: F401  (dbg900: the fixture of that file)

pytestmark = pytest.mark.gpu

NPTS = [16, 24, 64, 12]  # S = 2, 3, 8, and 12: one segment per run


@pytest.mark.parametrize("umr", [True, False])
@pytest.mark.parametrize("npt", NPTS)
def test_mixed_lengths(gpu_lib, monkeypatch, dbg900, npt, umr):
    """`first` lanes beside sparse-tail lanes, an incomplete last group; 1127 nodes: a ragged last run and segment"""
    arrays, reads = dbg900
    assert arrays.n_nodes % 2 and arrays.n_nodes % 3 and arrays.n_nodes % 8
    _pair(arrays, reads, umr, monkeypatch, npt, skipped=True)


@pytest.mark.parametrize("npt", NPTS)
def test_graph_that_is_no_dbg(gpu_lib, monkeypatch, npt):
    """the zoo graph: self-loop, parallel edge, a hub of 7 arms, a back edge 30 nodes upstream"""
    b = base_case("zoo")
    reads = _mix_lengths(list(b["reads"]), b["arrays"].param.n_warmup)
    for umr in (True, False):
        _pair(b["arrays"], reads, umr, monkeypatch, npt)


@pytest.mark.parametrize("npt", NPTS)
def test_tandem_repeat(gpu_lib, monkeypatch, npt):
    arrays, reads, sg, haps = dataset("u20", 40, read_len=200, max_reads=150)
    reads = _mix_lengths(list(reads), arrays.param.n_warmup)
    for umr in (True, False):
        _pair(arrays, reads, umr, monkeypatch, npt)


@pytest.mark.parametrize("npt", [24, 64])
def test_lds_dma(gpu_lib, monkeypatch, dbg900, npt):
    """hulls whose length is no multiple of the ring's depth, rows that issue nothing"""
    arrays, reads = dbg900
    for umr in (True, False):
        _pair(arrays, reads, umr, monkeypatch, npt, {"PHMM_BWD_DMA": "1"}, skipped=True)


@pytest.mark.parametrize("env", [{"PHMM_FORCE_RADIX": "1"}, {"PHMM_NO_RUNMAX": "1"}], ids=lambda e: "+".join(sorted(e)))
def test_column_selects(gpu_lib, monkeypatch, dbg900, env):
    """what reads whole columns of the emit-prob planes, the unwalked cells included, under both selects"""
    arrays, reads = dbg900
    for umr in (True, False):
        _pair(arrays, reads, umr, monkeypatch, 64, env, skipped=True)


def test_against_the_oracle(gpu_lib, oracle, monkeypatch, dbg900):
    """the pair is not merely equal to each other: backward totals against run_sparse_adaptive (tie-aware, 1e-6)"""
    arrays, reads = dbg900
    on, off = _pair(arrays, reads, True, monkeypatch, 64, skipped=True)
    om = oracle.Model(arrays)
    keep = [i for i in range(0, len(reads), 4) if not on["flags"][i] & _ffi.PHMM_READ_FORCED_SWITCH]
    keep += [i for i, r in enumerate(reads) if len(r) <= arrays.param.n_warmup + 3 and i not in keep]

    def want(i):
        return om.run_sparse_adaptive(reads[i], True).to_full_prob_backward()
    scores_tie_aware(oracle, on["lb"][keep], np.array([want(i) for i in keep]), lambda b: want(keep[b]))
    assert len(keep) >= 40


@pytest.fixture(scope="module")
def cfg1m_head():
    import bench
    arrays, reads, w = bench.build_workload("cfg1m", 0)
    return arrays, reads[:64]


@pytest.mark.parametrize("npt,bound", [(64, 0.75), (16, 0.57), (8, 0.50)])
def test_segments_are_skipped(gpu_lib, monkeypatch, cfg1m_head, npt, bound):
    """The first 64 reads of cfg1m, W = 64: cells(masks) / cells(no masks), cells = live lanes x rows walked.  The
    kernel's rule replayed on the oracle's backward tables of these reads (H from the non-zero nodes of the hand-over
    column, marks by successors within n_max_gaps + 2 hops, one group of 64 lanes, hull per run) gives

        npt   one mask per run   segments
        64    0.984              0.7065
        16    0.849              0.5293
         8    0.674              0.4638

    and each bound lies between the two."""
    arrays, reads = cfg1m_head
    on, off = _pair(arrays, reads, True, monkeypatch, npt)
    assert not np.any(on["flags"] & _ffi.PHMM_READ_DEFERRED)
    lens = np.array([len(r) for r in reads], dtype=np.int64)
    cols = on["cols"].astype(np.int64)
    dense = int(np.where(cols < lens, cols + 1, lens).sum()) * arrays.n_nodes
    share = on["cells"] / off["cells"]
    print(f"\nnpt {npt}: cells with masks {on['cells']}, without {off['cells']}, dense count {dense}, share {share:.4f}")
    assert off["cells"] == dense
    assert share < bound
