"""Transition posteriors over mapping lists (phmm_run_with_mapping_edges, PHMMModel.run_with_mapping_edge_freqs):
PHMMModel::run_with_mapping (freq.rs:72-76) of every read on its lists, then PHMMOutput::to_edge_and_init_freqs
(freq.rs:276-298, 332-389) summed over the reads.

Against the dense run where every node is listed (the two are the same sums then), the reference's own assertions,
and the oracle's run_with_mapping on the GPU's lists.  Small read sets only: the whole file is meant to take well under
a minute on the GPU."""
import json
import os

import numpy as np
import pytest

import dbgphmm_amd as D
from dbgphmm_amd import _ffi
from helpers import small_dbg_model, subset_csr
from repeat_cases import dataset

pytestmark = pytest.mark.gpu
KAT = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "kat_hmmv2.json")))
TOL_FREQ = 1e-9


def _all_nodes(rc, n_nodes):
    """every node listed at every position"""
    T = int(rc.offsets[-1])
    return D.Mappings.from_arrays(rc, np.arange(T + 1, dtype=np.uint64) * n_nodes, np.tile(np.arange(n_nodes), T))


def _oracle_sums(oracle, arrays, reads, rc, arr):
    """sum over the reads of the oracle's run_with_mapping(read, its lists).to_edge_and_init_freqs() -> (lf, ef, inf)"""
    om = oracle.Model(arrays)
    off = rc.offsets.astype(np.int64)
    lf, ef, inf = np.zeros(len(reads)), np.zeros(arrays.n_edges), np.zeros(arrays.n_nodes)
    for i, r in enumerate(reads):
        o = om.run_with_mapping(r, oracle.Mapping(*subset_csr(off, arr, [i])))
        lf[i] = o.to_full_prob_forward()
        e1, n1 = o.to_edge_and_init_freqs()
        ef += e1
        inf += n1
    return lf, ef, inf


def _check_oracle(oracle, arrays, reads, rc, mp):
    lf, ef, inf = D.PHMMModel(arrays).run_with_mapping_edge_freqs(rc, mp)
    olf, oef, oinf = _oracle_sums(oracle, arrays, reads, rc, mp.arrays())
    tol = TOL_FREQ * max(1, len(reads))
    assert np.max(np.abs(lf - olf)) < tol, np.max(np.abs(lf - olf))
    assert np.max(np.abs(ef - oef)) < tol, np.max(np.abs(ef - oef))
    assert np.max(np.abs(inf - oinf)) < tol, np.max(np.abs(inf - oinf))
    return lf, ef, inf


def _rel_close(a, b, rtol):
    return np.all(np.abs(a - b) <= rtol * np.maximum(np.abs(b), 1e-300) + 1e-300)


def test_linear_kats_every_node_listed(gpu_lib):
    """freq.rs:517-609 (test_edge_freq_kats) with every node listed: equal to the dense run."""
    for param, read in ((D.PHMMParams.zero_error(), b"CGATC"), (D.PHMMParams.default(), b"ATTCGTCGT")):
        arrays = D.mock_linear().to_phmm(param)
        gm = D.PHMMModel(arrays)
        rc = D.ReadCollection([read])
        lf, ef, inf = gm.run_with_mapping_edge_freqs(rc, _all_nodes(rc, arrays.n_nodes))
        dlf, def_, dinf = gm.run_dense_edge_freqs(rc)
        assert abs(lf[0] - dlf[0]) < 1e-9
        assert _rel_close(ef, def_, 1e-9) and _rel_close(inf, dinf, 1e-9)
        if read == b"CGATC":
            assert np.all(ef[[0, 1, 2, 7, 8]] < 1e-4) and np.all(ef[3:7] > 0.9999)
        else:
            assert np.allclose(ef, 0.99, atol=0.01)


def test_crossing_every_node_listed(gpu_lib):
    """seq_graph.rs:494-500: edge 37 is used (0.99992) without edge copy numbers; with them edges 37 and 38 are 0."""
    rb = KAT["crossing"]["read"].encode()
    for with_cn in (False, True):
        arrays = D.mock_crossing(with_cn).to_phmm(D.PHMMParams.default())
        gm = D.PHMMModel(arrays)
        rc = D.ReadCollection([rb])
        lf, ef, inf = gm.run_with_mapping_edge_freqs(rc, _all_nodes(rc, arrays.n_nodes))
        dlf, def_, dinf = gm.run_dense_edge_freqs(rc)
        assert abs(lf[0] - dlf[0]) < 1e-9
        assert _rel_close(ef, def_, 1e-9) and _rel_close(inf, dinf, 1e-9)
        if with_cn:
            assert ef[37] == 0.0 and ef[38] == 0.0
        else:
            assert abs(ef[37] - 0.99992) < 1e-5
            assert ef[36] < 1e-4 and ef[38] < 1e-4 and ef[39] < 1e-4


@pytest.mark.parametrize("n_reads", [1, 5, 70])
def test_generated_lists_match_oracle(gpu_lib, oracle, n_reads):
    """lists of generate_mappings(None) on the GPU; read lengths trimmed as in test_edge_and_init_freqs_match_oracle"""
    arrays, _ = small_dbg_model(300, 12, 0.01, seed=5)
    reads = D.sample_reads(arrays, 10 ** 9, 60, seed=n_reads, max_reads=n_reads)
    reads = [r[: max(1, len(r) - (j * 7) % 31)] for j, r in enumerate(reads)]
    rc = D.ReadCollection(reads)
    mp, _ = D.PHMMModel(arrays).generate_mappings(rc, None, True)
    lf, ef, inf = _check_oracle(oracle, arrays, reads, rc, mp)
    assert np.all(np.isfinite(ef)) and np.all(ef >= 0.0)
    # every read leaves the Begin states about once
    assert abs(inf.sum() - len(reads)) < 0.01 * len(reads)


def test_lists_of_the_400_slot_class(gpu_lib, oracle):
    """u20n200 (a 20 bp unit x 200 with 2 % divergence): lists longer than 64 nodes run in the 400-slot kernel"""
    arrays, reads, _, _ = dataset("u20n200", 40)
    rng = np.random.default_rng(5)
    reads = [reads[int(i)][:400] for i in rng.choice(len(reads), 3, replace=False)]
    rc = D.ReadCollection(reads)
    mp, _ = D.PHMMModel(arrays).generate_mappings(rc, None, True)
    po = mp.arrays()[0].astype(np.int64)
    assert np.max(np.diff(po)) > 64
    _check_oracle(oracle, arrays, reads, rc, mp)


def test_short_reads_on_hand_built_lists(gpu_lib, oracle):
    """reads under 100 bases, where the Begin terms over b_init's every node (both read ends) are not 0: lists are the
    oracle's dense posteriors cut to a per-read width (one-base and two-base reads included)"""
    arrays, _ = small_dbg_model(300, 12, 0.01, seed=5, min_copy_num=1)
    om = oracle.Model(arrays)
    reads = D.sample_reads(arrays, 10 ** 9, 60, seed=11, max_reads=8)
    reads = [reads[0][:1], reads[1][:2], reads[2][:5]] + [r[: 20 + 9 * j] for j, r in enumerate(reads[3:])]
    widths = [3, 1, 8, 12, 2, 40, 70, 5]
    po, nd = [0], []
    for r, w in zip(reads, widths):
        m = om.run(r).to_mapping(w)
        for i in range(len(r)):
            nodes = m.nodes(i)
            nd.extend(nodes)
            po.append(po[-1] + len(nodes))
    rc = D.ReadCollection(reads)
    mp = D.Mappings.from_arrays(rc, np.array(po, dtype=np.uint64), np.array(nd, dtype=np.uint32))
    lf, ef, inf = _check_oracle(oracle, arrays, reads, rc, mp)
    assert np.max(inf) > 1e-3


def test_refusals(gpu_lib):
    """a model that cuts a read on its lists (a zero-copy k-mer) and mappings of another read set are PHMM_EINVAL"""
    arrays, sg = small_dbg_model(900, 12, 0.003, seed=21, min_copy_num=1)
    reads = [r for r in D.sample_reads(arrays, 10 ** 9, 420, seed=21, max_reads=40) if len(r) > 380][:4]
    rc = D.ReadCollection(reads)
    gm = D.PHMMModel(arrays)
    mp, _ = gm.generate_mappings(rc, None, True)
    lf, _, _ = gm.run_with_mapping_edge_freqs(rc, mp)
    assert np.all(np.isfinite(lf))
    # every node listed at bases 300..305 of read 0 goes to copy number 0: the read is cut there, far past the point
    # where the InsBegin chain could carry it
    po, nd, _ = mp.arrays()
    p0 = int(rc.offsets[0])
    cn = sg.copy_num.copy()
    cn[np.unique(nd[int(po[p0 + 300]):int(po[p0 + 306])])] = 0
    with np.errstate(divide="ignore"):
        a2 = D.vectorised_to_phmm(D.SeqGraph(cn, sg.base, sg.edge_src, sg.edge_dst, None), arrays.param, 0)
    with pytest.raises(D.PhmmError, match="read 0"):
        D.PHMMModel(a2).run_with_mapping_edge_freqs(rc, mp)
    other = D.ReadCollection(reads[:1])
    with pytest.raises(D.PhmmError) as e:
        gm.run_with_mapping_edge_freqs(other, mp)
    assert e.value.code == _ffi.PHMM_EINVAL


class _DeviceArray:
    """a float64 array in device memory (the HIP runtime the library is linked against)"""

    def __init__(self, n):
        import ctypes as C
        self.C, self.hip, self.n = C, C.CDLL("libamdhip64.so"), n
        self.p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.p), C.c_size_t(8 * max(n, 1))) == 0

    def numpy(self):
        out = np.empty(self.n)
        assert self.hip.hipMemcpy(out.ctypes.data_as(self.C.c_void_p), self.p, self.C.c_size_t(8 * self.n), 2) == 0
        return out

    def __del__(self):
        self.hip.hipFree(self.p)


def test_output_forms_repeatability_and_q(gpu_lib, oracle):
    """device-pointer outputs equal host outputs, NULL outputs are allowed, two calls give the same bits, and
    q_score_exact (q.rs:66-96) on these freqs equals its value on the oracle's"""
    arrays, _ = small_dbg_model(300, 12, 0.01, seed=5, min_copy_num=1)
    reads = D.sample_reads(arrays, 10 ** 9, 60, seed=3, max_reads=20)
    rc = D.ReadCollection(reads)
    gm = D.PHMMModel(arrays)
    mp, _ = gm.generate_mappings(rc, None, True)
    lf, ef, inf = gm.run_with_mapping_edge_freqs(rc, mp)
    lf2, ef2, inf2 = gm.run_with_mapping_edge_freqs(rc, mp)
    assert np.array_equal(lf, lf2) and np.array_equal(ef, ef2) and np.array_equal(inf, inf2)
    L = _ffi.lib()
    dl, de, di = _DeviceArray(len(reads)), _DeviceArray(arrays.n_edges), _DeviceArray(arrays.n_nodes)
    _ffi.check(L.phmm_run_with_mapping_edges(gm._h, rc._h, mp._h, dl.p, de.p, di.p))
    assert np.array_equal(dl.numpy(), lf) and np.array_equal(de.numpy(), ef) and np.array_equal(di.numpy(), inf)
    _ffi.check(L.phmm_run_with_mapping_edges(gm._h, rc._h, mp._h, None, None, None))
    e_only = np.empty(arrays.n_edges)
    _ffi.check(L.phmm_run_with_mapping_edges(gm._h, rc._h, mp._h, None, e_only.ctypes.data_as(_ffi.C.c_void_p), None))
    assert np.array_equal(e_only, ef)
    _, oef, oinf = _oracle_sums(oracle, arrays, reads, rc, mp.arrays())
    q, oq = gm.q_score_exact(ef, inf), gm.q_score_exact(oef, oinf)
    for a, b in zip(q, oq):
        assert abs(a - b) <= 1e-9 * max(1.0, abs(b)), (q, oq)
