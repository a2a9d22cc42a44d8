"""GPU: draws from the posterior over paths of every read over its mapping lists (phmm_run_with_mapping_sample_paths,
PHMMModel.run_with_mapping_sample_paths).

The call is held to tests/sample_paths_ref.py, the header's sums, random stream and draw rule in plain Python (held on
its own by tests/test_sample_paths_ref_cpu.py):
  * out_path equals the restatement's rows WORD FOR WORD for every read and sample of the shared fixtures.  The
    device's exp / log and Python's may differ in the last bits of the forward values, so this needs every decision to
    stay clear of its boundaries: the CPU test asserts a margin of 1e-9 of every fixture (a condition on the inputs);
  * out_counts equals what score_path counts on those rows, out_path_logp is score_path's re-scored value within
    best_path_ref.bar (4 n_terms 2^-53 |ln P|; where a walk took the lighter of two parallel edges, which the rows
    cannot show and score_path re-scores over the heavier, plus the difference of the two edges), out_logp is the
    oracle's forward_score_only over the lists as sets within 1e-9;
  * the path counts of 40 000 walks pass the chi-square against the exact law; the emitting-state frequencies agree
    with run_with_mapping_states; out_node_usage is a recount of out_path;
  * a read's bits do not depend on the other reads, the capacity class, chunks, or where the outputs live."""
import ctypes as C
import math

import numpy as np
import pytest

import dbgphmm_amd as D
import best_path_ref as B
import sample_paths_ref as S
from dbgphmm_amd import _ffi
from graph_cases import zoo_graph, zoo_model

pytestmark = pytest.mark.gpu
NONE, NINF = S.NONE, -math.inf
STATS_HINTED = 2


def _call(gm, reads, lists, n_samples, seed, **kw):
    """one call with lists[read][pos] -> (rc, mp, logp, path_logp, path, counts, usage)"""
    rc = D.ReadCollection(reads)
    po, nd = B.csr(lists)
    mp = D.Mappings.from_arrays(rc, po, nd)
    lp, plp, path, counts, usage = gm.run_with_mapping_sample_paths(rc, mp, n_samples, seed, **kw)
    assert lp.shape == (len(reads),) and plp.shape == (len(reads), n_samples) and counts.shape == (len(reads), n_samples, 4)
    if path is not None:
        assert path.shape == (n_samples, rc.total_bases(), gm.param.n_max_gaps + 2)
    return rc, mp, lp, plp, path, counts, usage


def _same_bits(x, y):
    return all((a is None and b is None) or np.array_equal(a, b, equal_nan=True) for a, b in zip(x, y))


def _as_set(lst):
    seen, out = set(), []
    for v in lst:
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


# ------------------------------------------------------------------ 1. word for word against the restatement
N_ODD = len(S.odd_cases("ord"))


def _fixture_ids():
    return ["dbg", "zoo", "linear"] + [f"odd{k}" for k in range(N_ODD)]


@pytest.mark.parametrize("k", range(3 + N_ODD), ids=_fixture_ids())
def test_word_for_word(gpu_lib, oracle, k):
    f = S.fixtures()[k]
    arrays, reads, lists, n, seed = f["arrays"], f["reads"], f["lists"], f["n_samples"], f["seed"]
    want = S.fixture_samples(k)
    gm = D.PHMMModel(arrays)
    rc, mp, lp, plp, path, counts, usage = _call(gm, reads, lists, n, seed, want_usage=True)
    om = oracle.Model(arrays)
    off = rc.offsets.astype(np.int64)
    worst_z = worst_p = 0.0
    finite = 0
    for j, (r, ls) in enumerate(zip(reads, lists)):
        total = om.forward_score_only(r, oracle.Mapping.from_lists([_as_set(x) for x in ls]))
        if total == NINF or lp[j] == NINF:
            assert lp[j] == total == want[j]["logz"], (f["tag"], j, lp[j], total)
            assert np.all(path[:, off[j]:off[j + 1]] == NONE) and np.all(plp[j] == NINF) and not counts[j].any()
            continue
        finite += 1
        worst_z = max(worst_z, abs(lp[j] - total))
        assert abs(lp[j] - total) <= 1e-9, (f["tag"], j, lp[j], total)
        for s in range(n):
            rows = path[s, off[j]:off[j + 1]]
            if not np.array_equal(rows, want[j]["rows"][s]):
                raise AssertionError(f"{f['tag']}: " + S.first_difference(arrays, r, ls, j, s, seed, rows))
            v, n_terms, cnt = S.score_path(arrays, r, ls, rows)
            assert cnt == counts[j, s].tolist(), (f["tag"], j, s, cnt, counts[j, s].tolist())
            b = S.bar(n_terms, v)
            gap = abs(plp[j, s] - (v + want[j]["corr"][s]))
            worst_p = max(worst_p, gap / b)
            assert gap <= b, (f["tag"], j, s, plp[j, s], v, want[j]["corr"][s], b)
    print(f"{f['tag']}: {finite} of {len(reads)} reads have a path, {n} samples each equal word for word; "
          f"|out_logp - forward_score_only| at most {worst_z:.3e}, |out_path_logp - re-scored| at most {worst_p:.3f} of the bar")
    for s in range(n):
        assert np.array_equal(usage[s], S.usage_of(path[s], reads, lists, arrays.n_nodes)), (f["tag"], s)


# ------------------------------------------------------------------ 2. the exact law
@pytest.mark.parametrize("read", S.CHI_READS)
def test_chi_square_of_the_gpus_rows(gpu_lib, read):
    arrays, _ = S.chi_case()
    ls = S.full_lists(arrays, read)
    gm = D.PHMMModel(arrays)
    rc, mp, lp, plp, path, counts, _ = _call(gm, [read] * S.CHI_COPIES, [ls] * S.CHI_COPIES, S.CHI_SAMPLES, S.CHI_SEED)
    L = len(read)
    walks = [path[s, j * L:(j + 1) * L] for j in range(S.CHI_COPIES) for s in range(S.CHI_SAMPLES)]
    assert len(walks) == 40000 and np.all(lp == lp[0])
    chi, df, distinct = S.chi_square(arrays, read, ls, float(lp[0]), walks)
    print(f"{read}: {distinct} distinct paths, chi-square {chi:.1f} at df {df}, bar {S.chi_bar(df):.1f}")
    assert df >= 50 and chi <= S.chi_bar(df)


# ------------------------------------------------------------------ 3. against the state posteriors, and the usage
@pytest.fixture(scope="module")
def consistency_run(gpu_lib):
    c = S.consistency_case()
    gm = D.PHMMModel(c["arrays"])
    return (c, gm) + _call(gm, c["reads"], c["lists"], c["n_samples"], c["seed"], want_usage=True)


def test_state_frequencies_match_run_with_mapping_states(consistency_run):
    c, gm, rc, mp, lp, plp, path, counts, usage = consistency_run
    _, sl, _ = gm.run_with_mapping_states(rc, mp, want_best=False)
    po, _, _ = mp.arrays()
    off = rc.offsets.astype(np.int64)
    K = S.CONSISTENCY_COPIES
    worst, n_states = 0.0, 0
    for j in range(0, len(c["reads"]), K):
        read, ls = c["reads"][j], c["lists"][j]
        planes = [path[:, off[j + i]:off[j + i + 1]] for i in range(K)]
        freq, n = S.emitting_frequencies(planes, len(read), [len(x) for x in ls])
        assert n == K * c["n_samples"]
        for p in range(len(read)):
            e0 = int(po[off[j] + p])
            for slot in range(len(ls[p])):
                for kind in (0, 1):
                    prob = math.exp(sl[e0 + slot, kind])
                    gap = abs(freq[p][slot, kind] - prob)
                    worst = max(worst, gap / S.binomial_bar(prob, n))
                    n_states += 1
                    assert gap <= S.binomial_bar(prob, n), (j, p, slot, kind, freq[p][slot, kind], prob)
    print(f"{n_states} emitting states: the largest gap is {worst:.3f} of its bar")


def test_usage_is_a_recount_and_want_path_false_keeps_the_bits(consistency_run):
    c, gm, rc, mp, lp, plp, path, counts, usage = consistency_run
    for s in (0, 1, 31, 63):
        assert np.array_equal(usage[s], S.usage_of(path[s], c["reads"], c["lists"], c["arrays"].n_nodes)), s
    assert int(usage.sum()) == int(((path != NONE) & (path != S.INS_BEGIN)).sum())
    lp2, plp2, none, counts2, usage2 = gm.run_with_mapping_sample_paths(rc, mp, c["n_samples"], c["seed"], want_path=False,
                                                                        want_usage=True)
    assert none is None and _same_bits((lp, plp, counts, usage), (lp2, plp2, counts2, usage2))
    # copies of a read differ from each other: the read index is part of the stream
    off = rc.offsets.astype(np.int64)
    assert not np.array_equal(path[:, off[0]:off[1]], path[:, off[1]:off[2]])


# ------------------------------------------------------------------ 4. the same bits whatever surrounds a read
@pytest.fixture(scope="module")
def zoo_run(gpu_lib):
    f = S.graph_fixture("zoo")
    gm = D.PHMMModel(f["arrays"])
    return (f, gm) + _call(gm, f["reads"], f["lists"], 64, f["seed"], want_usage=True)


def test_a_read_alone_and_inside_a_larger_call(zoo_run):
    """the stream goes by the read's index, so read j alone (index 0) has the bits of read 0 of a call whose first read
    it is: the set rotated so that read j comes first gives read j the bits it has alone"""
    f, gm, rc, mp, lp, plp, path, counts, usage = zoo_run
    reads, lists = f["reads"], f["lists"]
    for j in (0, 5, 11):
        _, _, lp1, plp1, path1, counts1, _ = _call(gm, [reads[j]], [lists[j]], 64, f["seed"])
        rot_r, rot_l = reads[j:] + reads[:j], lists[j:] + lists[:j]
        _, _, lp2, plp2, path2, counts2, _ = _call(gm, rot_r, rot_l, 64, f["seed"])
        n = len(reads[j])
        assert lp1[0] == lp2[0] == lp[j]
        assert np.array_equal(plp1[0], plp2[0]) and np.array_equal(counts1[0], counts2[0])
        assert np.array_equal(path1, path2[:, :n])
    # and with the same index inside a larger call: the set with more reads behind it
    _, _, lp3, plp3, path3, counts3, _ = _call(gm, reads + reads[:4], lists + lists[:4], 64, f["seed"])
    R, nb = len(reads), path.shape[1]
    assert _same_bits((lp, plp, counts, path), (lp3[:R], plp3[:R], counts3[:R], path3[:, :nb]))


def _padded_sets():
    """-> [(tag, arrays with isolated nodes, first isolated node, reads, lists, seed)]: the zoo fixture and two odd-list
    groups (duplicates and empty lists among them)"""
    f = S.graph_fixture("zoo")
    out = [("zoo", S.with_isolated(f["arrays"]), f["arrays"].n_nodes, f["reads"][:6], f["lists"][:6], f["seed"])]
    for g in S.odd_cases("ord")[1:3]:
        out.append((g["tag"], S.with_isolated(g["arrays"]), g["arrays"].n_nodes, g["reads"], g["lists"], S.SEEDS["odd"]))
    return out


@pytest.mark.parametrize("which", range(3))
def test_unreachable_padding_same_bits(gpu_lib, which):
    """lists of the <= 64 class, then the same lists padded with isolated nodes (-inf in every state) behind their
    entries to 65, 129 and 400 and in front of them to 400: the 400 class returns the bits of the 64 class, with the
    slots shifted where the padding stands in front"""
    tag, arrays, first_pad, reads, lists, seed = _padded_sets()[which]
    gm = D.PHMMModel(arrays)
    n = 8
    rc, mp, lp, plp, path, counts, _ = _call(gm, reads, lists, n, seed)
    assert _ffi.last_call_stats(STATS_HINTED)[1] == 2
    off = rc.offsets.astype(np.int64)
    for width in (65, 129, 400):
        padded = [S.pad_unreachable(ls, first_pad, width, front=False) for ls in lists]
        _, _, lp2, plp2, path2, counts2, _ = _call(gm, reads, padded, n, seed)
        assert _ffi.last_call_stats(STATS_HINTED)[1] == 2
        assert _same_bits((lp, plp, path, counts), (lp2, plp2, path2, counts2)), (tag, width)
    padded = [S.pad_unreachable(ls, first_pad, 400, front=True) for ls in lists]
    _, _, lp3, plp3, path3, counts3, _ = _call(gm, reads, padded, n, seed)
    want = np.stack([np.concatenate([S.shift_slots(path[s, o:o + len(r)], ls, 400) for o, r, ls in zip(off, reads, lists)])
                     for s in range(n)])
    assert _same_bits((lp, plp, counts), (lp3, plp3, counts3)) and np.array_equal(path3, want), tag
    slots = path3[(path3 != NONE) & (path3 != S.INS_BEGIN)] >> 2
    assert int(slots.max()) > 255  # (chosen slots pass the 8 bits a narrower record could hold)


def test_both_classes_in_one_call_and_chunks(gpu_lib, zoo_run):
    """narrow and wide reads interleaved; then at least three chunks under a workspace limit"""
    f, gm0, rc0, mp0, lp0, plp0, path0, counts0, usage0 = zoo_run
    arrays = S.with_isolated(f["arrays"])
    reads = f["reads"]
    lists = [ls if j % 2 == 0 else S.pad_unreachable(ls, f["arrays"].n_nodes, 129, front=False) for j, ls in enumerate(f["lists"])]
    gm = D.PHMMModel(arrays)
    rc, mp, lp, plp, path, counts, usage = _call(gm, reads, lists, 64, f["seed"], want_usage=True)
    assert _ffi.last_call_stats(STATS_HINTED)[1] == 3  # the <= 64 class, the 400 class, the walk
    n_real = f["arrays"].n_nodes
    assert _same_bits((lp0, plp0, path0, counts0, usage0), (lp, plp, path, counts, usage[:, :n_real])) and not usage[:, n_real:].any()
    stride = path.shape[2]
    per_read = [128 * sum(len(x) for x in ls) + 8 * len(r) + 4 * stride * 64 * len(r) for r, ls in zip(reads, lists)]
    R = len(reads)
    fixed = 0
    for nbytes in (8 * R, 8 * (R + 1), 8 * R, 8 * R, 4 * R, 4 * R, 8 * R * 64, 16 * R * 64):  # the control arrays, each at a multiple of 256
        fixed = (fixed + 255) // 256 * 256 + nbytes
    fixed += 8 * (arrays.n_nodes + arrays.n_edges) + 4 * 64 * arrays.n_nodes
    limit = fixed + 2 * max(per_read)
    assert sum(per_read) > 2 * (2 * max(per_read))  # at least three chunks: no chunk holds more than 2 max(per_read)
    _ffi.check(gpu_lib.phmm_set_workspace_limit(limit))
    try:
        lp2, plp2, path2, counts2, usage2 = gm.run_with_mapping_sample_paths(rc, mp, 64, f["seed"], want_usage=True)
        launches = _ffi.last_call_stats(STATS_HINTED)[1]
    finally:
        _ffi.check(gpu_lib.phmm_set_workspace_limit(0))
    assert launches >= 6, launches  # three chunks or more: a forward class at least and a walk each
    assert _same_bits((lp, plp, path, counts, usage), (lp2, plp2, path2, counts2, usage2))


class _DeviceArray:
    """bytes in device memory (the HIP runtime the library is linked against)"""

    def __init__(self, nbytes, fill):
        self.hip, self.nbytes = C.CDLL("libamdhip64.so"), nbytes
        self.p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.p), C.c_size_t(max(nbytes, 1))) == 0
        assert self.hip.hipMemset(self.p, C.c_int(fill), C.c_size_t(max(nbytes, 1))) == 0

    def numpy(self, dtype):
        out = np.empty(self.nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        assert self.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), self.p, C.c_size_t(self.nbytes), 2) == 0
        return out

    def __del__(self):
        self.hip.hipFree(self.p)


def test_output_forms_and_a_second_call(gpu_lib, zoo_run):
    """device-pointer outputs equal host-pointer outputs bit for bit; every output may be NULL; a second identical call
    returns the same bits and allocates nothing; a call without reads writes nothing"""
    f, gm, rc, mp, lp, plp, path, counts, usage = zoo_run
    L, R, S_ = _ffi.lib(), len(rc), 64
    dl, dq, dp = _DeviceArray(lp.nbytes, 0x55), _DeviceArray(plp.nbytes, 0x55), _DeviceArray(path.nbytes, 0x55)
    dc, du = _DeviceArray(counts.nbytes, 0x55), _DeviceArray(usage.nbytes, 0x55)
    _ffi.check(L.phmm_run_with_mapping_sample_paths(gm._h, rc._h, mp._h, S_, f["seed"], dl.p, dq.p, dp.p, dc.p, du.p))
    assert np.array_equal(dl.numpy(np.float64), lp) and np.array_equal(dq.numpy(np.float64).reshape(plp.shape), plp)
    assert np.array_equal(dp.numpy(np.uint32).reshape(path.shape), path)
    assert np.array_equal(dc.numpy(np.uint32).reshape(counts.shape), counts)
    assert np.array_equal(du.numpy(np.uint32).reshape(usage.shape), usage)
    _ffi.check(L.phmm_run_with_mapping_sample_paths(gm._h, rc._h, mp._h, S_, f["seed"], None, None, None, None, None))
    second = gm.run_with_mapping_sample_paths(rc, mp, S_, f["seed"], want_usage=True)
    ws = gpu_lib.phmm_workspace_bytes()
    third = gm.run_with_mapping_sample_paths(rc, mp, S_, f["seed"], want_usage=True)
    assert gpu_lib.phmm_workspace_bytes() == ws
    assert _same_bits((lp, plp, path, counts, usage), second) and _same_bits(second, third)
    rc0 = D.ReadCollection([])
    mp0 = D.Mappings.from_arrays(rc0, np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint32))
    out = np.full(4, 7.5)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    _ffi.check(L.phmm_run_with_mapping_sample_paths(gm._h, rc0._h, mp0._h, 4, 1, P(out), P(out), None, None, None))
    assert np.all(out == 7.5)


def test_same_handle_new_numbers(gpu_lib):
    """after phmm_model_set_probs and phmm_model_set_params (n_max_gaps 2 -> 0) the bits of a fresh model"""
    g = [g for g in S.odd_cases("ord") if g["tag"].endswith("list oddities, n_max_gaps = 2")][0]
    a1, reads, lists = g["arrays"], g["reads"], g["lists"]
    # a2: other init and trans under the same parameters; a3: a2 under other parameters with n_max_gaps = 0
    a2 = D.PHMMArrays(a1.param, a1.emission, a1.init_logp + math.log(0.9), a1.edge_src, a1.edge_dst,
                      a1.trans_logp[::-1].copy())
    a3 = D.PHMMArrays(B.ordinary_params(0, p_MM=math.log(0.8)), a1.emission, a2.init_logp, a1.edge_src, a1.edge_dst, a2.trans_logp)
    gm = D.PHMMModel(a1)
    first = _call(gm, reads, lists, 5, 21)[2:]
    gm.set_probs(a2.init_logp, a2.trans_logp)
    got = _call(gm, reads, lists, 5, 21)[2:]
    assert _same_bits(got, _call(D.PHMMModel(a2), reads, lists, 5, 21)[2:]) and not np.array_equal(got[0], first[0])
    cp = a3.param.to_c()
    _ffi.check(_ffi.lib().phmm_model_set_params(gm._h, C.byref(cp)))
    gm.param = a3.param  # (PHMMModel sizes the rows by its param)
    got = _call(gm, reads, lists, 5, 21)[2:]
    assert got[2].shape[2] == 2
    assert _same_bits(got, _call(D.PHMMModel(a3), reads, lists, 5, 21)[2:])


def test_many_short_reads(gpu_lib, oracle):
    """320 reads of 1 to 12 bases, some lists with a duplicate: every walk is a legal path with the counts and the value
    the call reports, ln Z is the oracle's, and the reads keep their bits in chunks"""
    arrays, reads, lists = S.many_short_reads(320)
    gm = D.PHMMModel(arrays)
    n, seed = 2, 31
    rc, mp, lp, plp, path, counts, usage = _call(gm, reads, lists, n, seed, want_usage=True)
    assert len(reads) == 320 and _ffi.last_call_stats(STATS_HINTED)[1] == 2
    om = oracle.Model(arrays)
    off = rc.offsets.astype(np.int64)
    for j, (r, ls) in enumerate(zip(reads, lists)):
        total = om.forward_score_only(r, oracle.Mapping.from_lists([_as_set(x) for x in ls]))
        if total == NINF:
            assert lp[j] == NINF and np.all(path[:, off[j]:off[j + 1]] == NONE)
            continue
        assert abs(lp[j] - total) <= 1e-9, (j, lp[j], total)
        for s in range(n):
            v, n_terms, cnt = S.score_path(arrays, r, ls, path[s, off[j]:off[j + 1]])
            assert cnt == counts[j, s].tolist() and plp[j, s] <= v + S.bar(n_terms, v)
    for s in range(n):
        assert np.array_equal(usage[s], S.usage_of(path[s], reads, lists, arrays.n_nodes))
    stride = path.shape[2]
    per_read = [128 * sum(len(x) for x in ls) + 8 * len(r) + 4 * stride * n * len(r) for r, ls in zip(reads, lists)]
    _ffi.check(gpu_lib.phmm_set_workspace_limit((64 << 10) + sum(per_read) * 2 // 5))
    try:
        second = gm.run_with_mapping_sample_paths(rc, mp, n, seed, want_usage=True)
        launches = _ffi.last_call_stats(STATS_HINTED)[1]
    finally:
        _ffi.check(gpu_lib.phmm_set_workspace_limit(0))
    assert launches >= 4 and _same_bits((lp, plp, path, counts, usage), second)


# ------------------------------------------------------------------ 5. seeds and sample counts
def _status(f):
    try:
        f()
    except _ffi.PhmmError as e:
        return e.code
    return _ffi.PHMM_OK


def test_seeds_and_sample_counts(gpu_lib):
    arrays = S.linear(0.1)  # a high error rate: the walks spread
    reads = [b"ATTCGTCGT", b"ATTCA", b"GGATCTT"]
    lists = [S.full_lists(arrays, r) for r in reads]
    gm = D.PHMMModel(arrays)
    rc, mp, lp, plp, path, counts, _ = _call(gm, reads, lists, 64, 7)
    _, _, lp2, plp2, path2, counts2, _ = _call(gm, reads, lists, 64, 8)
    assert np.array_equal(lp, lp2) and not np.array_equal(path, path2)
    _, _, lp1, plp1, path1, counts1, _ = _call(gm, reads, lists, 1, 7)
    assert _same_bits((lp, plp[:, :1], path[:1], counts[:, :1]), (lp1, plp1, path1, counts1))
    L = _ffi.lib()
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    for n in (0, 65):
        o_lp, o_plp = np.full(3, 7.5), np.full((3, 65), 7.5)
        o_path = np.full((65, rc.total_bases(), 8), 77, dtype=np.uint32)
        o_cnt, o_use = np.full((3, 65, 4), 77, dtype=np.uint32), np.full((65, arrays.n_nodes), 77, dtype=np.uint32)
        rcode = L.phmm_run_with_mapping_sample_paths(gm._h, rc._h, mp._h, n, 7, P(o_lp), P(o_plp), P(o_path), P(o_cnt), P(o_use))
        assert rcode == _ffi.PHMM_EINVAL, (n, rcode)
        assert np.all(o_lp == 7.5) and np.all(o_plp == 7.5) and np.all(o_path == 77) and np.all(o_cnt == 77) and np.all(o_use == 77)


def test_refusals(gpu_lib, zoo_run):
    """those of the best-path call, each with sentinel-filled outputs unchanged"""
    f, gm, rc, mp, lp, plp, path, counts, usage = zoo_run
    L = _ffi.lib()
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    o_lp, o_path = np.full(len(rc), 7.5), np.full((2, rc.total_bases(), 8), 77, dtype=np.uint32)

    def call(m, r, p):
        return L.phmm_run_with_mapping_sample_paths(m, r, p, 2, 1, P(o_lp), None, P(o_path), None, None)
    for h in ((None, rc._h, mp._h), (gm._h, None, mp._h), (gm._h, rc._h, None)):
        assert call(*h) == _ffi.PHMM_EINVAL
    rc2 = D.ReadCollection(f["reads"][:2])
    assert call(gm._h, rc2._h, mp._h) == _ffi.PHMM_EINVAL  # mappings of another read set
    po, nd, _ = mp.arrays()
    bad = nd.copy()
    bad[len(bad) // 2] = f["arrays"].n_nodes
    assert call(gm._h, rc._h, D.Mappings.from_arrays(rc, po, bad)._h) == _ffi.PHMM_EINVAL  # a node out of range
    arrays, reads = B.width_reads(400)
    gw, rw = D.PHMMModel(arrays), D.ReadCollection(reads[:1])
    nb = rw.total_bases()

    def wide():  # (a list of 401 is refused where the lists are handed over)
        over = D.Mappings.from_arrays(rw, np.arange(nb + 1, dtype=np.uint64) * 401, np.tile(np.arange(401, dtype=np.uint32), nb))
        _ffi.check(call(gw._h, rw._h, over._h))
    assert _status(wide) == _ffi.PHMM_ECAPACITY
    # the degree limit: a hub of 9 arms
    hub, rch = D.PHMMModel(zoo_model(zoo_graph(arms=9))), D.ReadCollection([b"ACGTACGT"])
    mph = D.Mappings.from_arrays(rch, np.arange(9, dtype=np.uint64) * 3, np.tile(np.array([59, 60, 61], dtype=np.uint32), 8))
    assert call(hub._h, rch._h, mph._h) == _ffi.PHMM_EINVAL
    assert np.all(o_lp == 7.5) and np.all(o_path == 77)


# ------------------------------------------------------------------ 6. the bound
def test_no_sample_beats_the_best_path(zoo_run):
    f, gm, rc, mp, lp, plp, path, counts, usage = zoo_run
    best, _, _ = gm.run_with_mapping_best_path(rc, mp, want_path=False)
    off = rc.offsets.astype(np.int64)
    top = NINF
    for j, (r, ls) in enumerate(zip(f["reads"], f["lists"])):
        for s in range(64):
            v, n_terms, cnt = S.score_path(f["arrays"], r, ls, path[s, off[j]:off[j + 1]])  # (raises if the path is illegal)
            b = S.bar(n_terms, v)
            assert v <= best[j] + b and plp[j, s] <= best[j] + b and plp[j, s] <= lp[j] + b, (j, s, v, plp[j, s], best[j])
            top = max(top, v - best[j])
    print(f"the best sampled path is {top:.3e} from the best path")
