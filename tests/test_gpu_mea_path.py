"""GPU: the weighted walk over mapping lists and the maximum-expected-accuracy path built on it
(phmm_run_with_mapping_weighted_path, phmm_run_with_mapping_mea_path, include/phmm_amd_mea.h).

The weighted walk is held to tests/mea_path_ref.py (held on its own by tests/test_mea_path_ref_cpu.py): per read
out_score equal as a double, out_path and out_counts word for word -- the kernel and the restatement do the same double
additions in the same order, a maximum does not round, and the tie rule leaves one path.  Three kinds of weights: random
doubles, random multiples of 1/4 (exact sums: ties everywhere) and all zeros (the tie rule alone).  Within a call read j
takes kind (j + shift) % 3, and the small fixtures run every shift, so that every read meets every kind there; the
fixtures whose restatement takes seconds in Python run one shift.

The MEA call is held to the weighted walk on the weights it returns (the same bits), to the states call (its ln P bit for
bit, its weights against numpy.exp within 4 * 2^-52 relative: each side's exp is documented to within 1 ulp = 2^-52
relative, both ways) and to invariants that need no reference."""
import ctypes as C

import numpy as np
import pytest

import dbgphmm_amd as D
import best_path_ref as B
import caller_cases as cc
import mea_path_ref as M
from dbgphmm_amd import _ffi, _ffi_mea
from graph_cases import ORDERINGS, base_case, carry_mappings, relabelled_case, with_gaps, zoo_graph, zoo_model

pytestmark = pytest.mark.gpu
NONE = B.NONE
STATS_HINTED = 2
KINDS = ("random", "dyadic", "zeros")
EXP_BAR = 4.0 * 2.0 ** -52


def _P(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _weights(rng, kind, shape):
    if kind == "random":
        return rng.normal(size=shape) * 10.0 ** rng.integers(-2, 3, size=shape)
    if kind == "dyadic":
        return M.dyadic(rng, shape)
    return np.zeros(shape)


def _mixed(seed, shift, rc, po, with_ib):
    """weights of a whole call: read j takes kind (j + shift) % 3 -> (weights[total_entries, 3], ib_weight or None, kinds)"""
    rng = np.random.default_rng([20261105, seed, shift])
    off = rc.offsets.astype(np.int64)
    w, ib, kinds = np.zeros((int(po[-1]), 3)), np.zeros(int(off[-1])), []
    for j in range(len(rc)):
        kind = KINDS[(j + shift) % 3]
        e0, e1 = int(po[off[j]]), int(po[off[j + 1]])
        w[e0:e1] = _weights(rng, kind, (e1 - e0, 3))
        ib[off[j]:off[j + 1]] = _weights(rng, kind, int(off[j + 1] - off[j]))
        kinds.append(kind)
    return w, (ib if with_ib else None), kinds


def _handles(arrays, reads, lists=None):
    """-> (model, reads, mappings, pos_off, nodes); lists = (pos_off, nodes) or None for the model's own generate_mappings"""
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    mp = gm.generate_mappings(rc, None, True)[0] if lists is None else D.Mappings.from_arrays(rc, lists[0], lists[1])
    po, nd, _ = mp.arrays()
    return gm, rc, mp, po, nd


def _hold(arrays, reads, rc, po, nd, w, ib, score, path, counts, what):
    """every read against the restatement -> how many reads have a path"""
    off = rc.offsets.astype(np.int64)
    assert path.shape == (rc.total_bases(), arrays.param.n_max_gaps + 2) and counts.shape == (len(reads), 4)
    finite = 0
    for j, r in enumerate(reads):
        e0, e1 = int(po[off[j]]), int(po[off[j + 1]])
        want = M.check_read(arrays, r, B.lists_of(po, nd, off[j], off[j + 1]), w[e0:e1],
                            None if ib is None else ib[off[j]:off[j + 1]], float(score[j]), path[off[j]:off[j + 1]],
                            counts[j].tolist())
        finite += want > -np.inf
    print(f"{what}: {len(reads)} reads, {finite} with a path")
    return finite


def _parity(arrays, reads, lists=None, shifts=(0, 1, 2), seed=0, what=""):
    gm, rc, mp, po, nd = _handles(arrays, reads, lists)
    out = None
    for shift in shifts:
        w, ib, _ = _mixed(seed, shift, rc, po, with_ib=shift != 1)
        score, path, counts = gm.run_with_mapping_weighted_path(rc, mp, w, ib)
        _hold(arrays, reads, rc, po, nd, w, ib, score, path, counts, f"{what}, shift {shift}")
        out = (gm, rc, mp, po, nd, w, ib, score, path, counts)
    return out


def _same_bits(x, y):
    return all(cc.same_bits(np.asarray(a), np.asarray(b)) for a, b in zip(x, y))


# ------------------------------------------------------------------ 1. the weighted walk against the restatement
def test_linear_mock(gpu_lib):
    """10 nodes; with errors on the model's own lists, and without errors on full lists, where CGATT has no path"""
    _parity(B.linear(0.01), [b"ATTCGTCGT", b"ATTCGCATCGT", b"ATTCGATGGT"], what="linear mock, uniform(0.01)")
    a = B.linear(0.0)
    reads = [b"CGATC", b"CGATT"]
    n = sum(len(r) for r in reads)
    full = (np.arange(n + 1, dtype=np.uint64) * a.n_nodes, np.tile(np.arange(a.n_nodes, dtype=np.uint32), n))
    gm, rc, mp, po, nd, w, ib, score, path, counts = _parity(a, reads, full, what="linear mock, uniform(0)")
    assert np.isfinite(score[0]) and score[1] == -np.inf and np.all(path[5:] == NONE) and counts[1].tolist() == [0, 0, 0, 0]
    assert D.path_states(mp, 0, path) == [(v, "M") for v in range(3, 8)] and D.path_states(mp, 1, path) == []


@pytest.mark.parametrize("graph", ["zoo", "dbg"])
def test_parity_small_graphs(gpu_lib, graph):
    b = base_case(graph)
    _parity(b["arrays"], b["reads"], seed=1, what=graph)


@pytest.mark.parametrize("which", range(6))
def test_parity_fuzz(gpu_lib, which):
    c = B.fuzz_cases()[which]
    _parity(c["arrays"], c["reads"], shifts=(which % 3,), seed=2 + which, what=c["tag"])


@pytest.mark.parametrize("gaps", [0, 4, 6])
def test_del_levels(gpu_lib, gaps):
    """zero weights but for the Del column at 1: the path collects Dels, up to n_max_gaps + 1 behind a base"""
    arrays, read = B.two_deletions()
    a = with_gaps(arrays, gaps)
    _parity(a, [read], seed=10 + gaps, what=f"n_max_gaps = {gaps}")
    gm, rc, mp, po, nd = _handles(a, [read])
    w = np.zeros((int(po[-1]), 3))
    w[:, 2] = 1.0
    score, path, counts = gm.run_with_mapping_weighted_path(rc, mp, w)
    _hold(a, [read], rc, po, nd, w, None, score, path, counts, f"Del weights, n_max_gaps = {gaps}")
    assert path.shape[1] == gaps + 2 and score[0] == counts[0, 3] > 0


def _gpu_lists(arrays, reads):
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    po, nd, _ = gm.generate_mappings(rc, None, True)[0].arrays()
    return po, nd


@pytest.mark.parametrize("width", B.WIDTHS)
def test_list_widths(gpu_lib, width):
    arrays, reads = B.width_reads(width)
    po0, nd0 = _gpu_lists(arrays, reads)
    ppo, pnd = B.pad_lists(po0, nd0, reads, arrays.n_nodes, width)
    assert int(np.diff(ppo.astype(np.int64)).max()) == width
    out = _parity(arrays, reads, (ppo, pnd), shifts=(B.WIDTHS.index(width) % 3,), seed=20, what=f"lists padded to {width}")
    assert np.all(np.isfinite(out[7]))
    ms, launches, cells = _ffi.last_call_stats(STATS_HINTED)
    assert cells == int(ppo[-1]) and launches == 2  # one capacity class and the walk back


@pytest.mark.parametrize("flavour", ["ord", "int"])
def test_odd_lists(gpu_lib, flavour):
    """duplicated entries, empty lists, reads of one base, each parameter at -inf, init on one node, the forced forms"""
    n = finite = 0
    for k, g in enumerate(B.odd_cases(flavour)):
        po, nd = B.csr(g["lists"])
        gm, rc, mp, po, nd = _handles(g["arrays"], g["reads"], (po, nd))
        for shift in (0, 1, 2):
            w, ib, _ = _mixed(30 + k, shift, rc, po, with_ib=shift != 2)
            score, path, counts = gm.run_with_mapping_weighted_path(rc, mp, w, ib)
            f = _hold(g["arrays"], g["reads"], rc, po, nd, w, ib, score, path, counts, f"{g['tag']}, shift {shift}")
        n, finite = n + len(score), finite + f
    assert 2 * finite >= n and finite < n


def test_both_classes_in_one_call_and_chunks(gpu_lib):
    c = B.int_case("zoo")
    arrays, reads = c["arrays"], c["reads"]
    lists = [ls if j % 2 == 0 else B.pad_unreachable(ls, c["n_real"], 129, front=False) for j, ls in enumerate(c["lists"])]
    gm, rc, mp, po, nd, w, ib, score, path, counts = _parity(arrays, reads, B.csr(lists), shifts=(2,), seed=40,
                                                             what="narrow and wide reads interleaved")
    assert _ffi.last_call_stats(STATS_HINTED)[1] == 3  # the <= 64 class, the 400 class, the walk
    # a read alone equals that read in the batch
    off = rc.offsets.astype(np.int64)
    for j in (0, 1, len(reads) - 1):
        rc1 = D.ReadCollection([reads[j]])
        e0, e1 = int(po[off[j]]), int(po[off[j + 1]])
        mp1 = D.Mappings.from_arrays(rc1, po[off[j]:off[j + 1] + 1] - po[off[j]], nd[e0:e1])
        s1, p1, c1 = gm.run_with_mapping_weighted_path(rc1, mp1, w[e0:e1], ib[off[j]:off[j + 1]])
        assert _same_bits((s1[0], p1, c1[0]), (score[j], path[off[j]:off[j + 1]], counts[j])), j
    # chunks: the uploaded weights and the call's fixed arrays, then records and staged rows of two reads or more
    per_read = [16 * sum(len(x) for x in ls) + 4 * path.shape[1] * len(r) for r, ls in zip(reads, lists)]
    limit = w.nbytes + ib.nbytes + 2 * max(per_read) + (64 << 10)
    assert sum(per_read) > 2 * (2 * max(per_read) + (64 << 10))  # at least three chunks
    _ffi.check(gpu_lib.phmm_set_workspace_limit(limit))
    try:
        got = gm.run_with_mapping_weighted_path(rc, mp, w, ib)
        launches = _ffi.last_call_stats(STATS_HINTED)[1]
    finally:
        _ffi.check(gpu_lib.phmm_set_workspace_limit(0))
    assert launches >= 6 and _same_bits(got, (score, path, counts))
    # a second call returns the same bits
    assert _same_bits(gm.run_with_mapping_weighted_path(rc, mp, w, ib), (score, path, counts))
    s3, none, c3 = gm.run_with_mapping_weighted_path(rc, mp, w, ib, want_path=False)
    assert none is None and _same_bits((s3, c3), (score, counts))


def test_many_short_reads(gpu_lib):
    """320 reads: five blocks of the walk back and two of the entry offsets"""
    arrays, reads, lists = B.many_short_reads()
    assert len(reads) > 256
    _parity(arrays, reads, B.csr(lists), shifts=(2,), seed=50, what=f"{len(reads)} short reads")
    assert _ffi.last_call_stats(STATS_HINTED)[1] == 2


def test_long_read(gpu_lib):
    arrays, read = B.long_read()
    assert len(read) == 3000
    out = _parity(arrays, [read], shifts=(1,), seed=60, what="one read of 3000 bases")  # (shift 1: read 0 is dyadic)
    assert np.isfinite(out[7][0])


# ------------------------------------------------------------------ 2. refusals
class _Prefilled:
    """sentinel-filled outputs of one call"""

    def __init__(self, rc, te, stride=8):
        self.lf = np.full(max(len(rc), 1), 7.5)
        self.score = np.full(max(len(rc), 1), 7.5)
        self.path = np.full((max(rc.total_bases(), 1), stride), 77, dtype=np.uint32)
        self.counts = np.full((max(len(rc), 1), 4), 77, dtype=np.uint32)
        self.w = np.full((max(te, 1), 3), 7.5)

    def walk(self, gm, rc, mp, w, ib=None):
        _ffi.check(_ffi_mea.lib().phmm_run_with_mapping_weighted_path(gm._h, rc._h, mp._h, _P(w), _P(ib), _P(self.score),
                                                                      _P(self.path), _P(self.counts)))

    def mea(self, gm, rc, mp, del_weight=1.0):
        _ffi.check(_ffi_mea.lib().phmm_run_with_mapping_mea_path(gm._h, rc._h, mp._h, del_weight, _P(self.lf), _P(self.score),
                                                                 _P(self.path), _P(self.counts), _P(self.w)))

    def untouched(self):
        return bool(np.all(self.lf == 7.5) and np.all(self.score == 7.5) and np.all(self.path == 77)
                    and np.all(self.counts == 77) and np.all(self.w == 7.5))


def _status(f):
    try:
        f()
    except _ffi.PhmmError as e:
        return e.code
    return _ffi.PHMM_OK


@pytest.fixture(scope="module")
def dbg(gpu_lib):
    b = base_case("dbg")
    return (b,) + _handles(b["arrays"], b["reads"])


def test_refusals(gpu_lib, dbg):
    b, gm, rc, mp, po, nd = dbg
    L = _ffi_mea.lib()
    te = int(po[-1])
    w = np.random.default_rng(70).normal(size=(te, 3))
    out = _Prefilled(rc, te)
    out.walk(gm, rc, mp, w)  # (the call itself is fine)
    assert not out.untouched()
    out = _Prefilled(rc, te)
    # a list of 401 nodes
    arrays, reads = B.width_reads(400)
    gm4, rc4 = D.PHMMModel(arrays), D.ReadCollection(reads)
    n = rc4.total_bases()
    out4 = _Prefilled(rc4, 401 * n)

    def over():  # (a list of 401 is refused where the lists are handed over)
        return D.Mappings.from_arrays(rc4, np.arange(n + 1, dtype=np.uint64) * 401, np.tile(np.arange(401, dtype=np.uint32), n))
    assert _status(lambda: out4.walk(gm4, rc4, over(), np.zeros((401 * n, 3)))) == _ffi.PHMM_ECAPACITY
    assert _status(lambda: out4.mea(gm4, rc4, over())) == _ffi.PHMM_ECAPACITY and out4.untouched()
    # a weight that is NaN, +inf, -inf; an InsBegin weight that is NaN; weights == NULL
    for bad in (np.nan, np.inf, -np.inf):
        wb = w.copy()
        wb[te // 2, 1] = bad
        assert _status(lambda: out.walk(gm, rc, mp, wb)) == _ffi.PHMM_EINVAL, bad
    wb = w.copy()
    wb[-1, 2] = np.nan  # (the last double of the plane)
    assert _status(lambda: out.walk(gm, rc, mp, wb)) == _ffi.PHMM_EINVAL
    ibb = np.zeros(rc.total_bases())
    ibb[3] = np.nan
    assert _status(lambda: out.walk(gm, rc, mp, w, ibb)) == _ffi.PHMM_EINVAL
    assert _status(lambda: out.walk(gm, rc, mp, None)) == _ffi.PHMM_EINVAL
    # a node out of range, NULL handles, mappings of another read set
    badn = nd.copy()
    badn[len(badn) // 2] = b["arrays"].n_nodes
    mpb = D.Mappings.from_arrays(rc, po, badn)
    assert _status(lambda: out.walk(gm, rc, mpb, w)) == _ffi.PHMM_EINVAL
    assert _status(lambda: out.mea(gm, rc, mpb)) == _ffi.PHMM_EINVAL
    for h in ((None, rc._h, mp._h), (gm._h, None, mp._h), (gm._h, rc._h, None)):
        assert L.phmm_run_with_mapping_weighted_path(*h, _P(w), None, _P(out.score), _P(out.path), _P(out.counts)) == _ffi.PHMM_EINVAL
        assert L.phmm_run_with_mapping_mea_path(*h, 1.0, _P(out.lf), _P(out.score), _P(out.path), _P(out.counts), _P(out.w)) == _ffi.PHMM_EINVAL
    rc2 = D.ReadCollection(b["reads"][:2])
    assert _status(lambda: out.walk(gm, rc2, mp, w)) == _ffi.PHMM_EINVAL
    # the degree limit: a hub of 9 arms
    hub, rch = D.PHMMModel(zoo_model(zoo_graph(arms=9))), D.ReadCollection([b"ACGTACGT"])
    mph = D.Mappings.from_arrays(rch, np.arange(9, dtype=np.uint64) * 3, np.tile(np.array([59, 60, 61], dtype=np.uint32), 8))
    outh = _Prefilled(rch, 24)
    assert _status(lambda: outh.walk(hub, rch, mph, np.zeros((24, 3)))) == _ffi.PHMM_EINVAL and outh.untouched()
    # del_weight
    for dw in (-1.0, np.nan, np.inf):
        assert _status(lambda: out.mea(gm, rc, mp, dw)) == _ffi.PHMM_EINVAL, dw
    assert out.untouched()
    # every output may be NULL; no reads: nothing is written
    _ffi.check(L.phmm_run_with_mapping_weighted_path(gm._h, rc._h, mp._h, _P(w), None, None, None, None))
    _ffi.check(L.phmm_run_with_mapping_mea_path(gm._h, rc._h, mp._h, 1.0, None, None, None, None, None))
    rc0 = D.ReadCollection([])
    mp0 = D.Mappings.from_arrays(rc0, np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint32))
    out0 = _Prefilled(rc0, 0)
    out0.walk(gm, rc0, mp0, np.zeros((1, 3)))
    out0.mea(gm, rc0, mp0)
    assert out0.untouched()


def test_a_read_of_probability_zero_is_refused_by_the_mea_call(gpu_lib):
    a = B.linear(0.0)
    reads = [b"CGATC", b"CGATT"]
    n = sum(len(r) for r in reads)
    gm, rc, mp, po, nd = _handles(a, reads, (np.arange(n + 1, dtype=np.uint64) * a.n_nodes,
                                             np.tile(np.arange(a.n_nodes, dtype=np.uint32), n)))
    out = _Prefilled(rc, int(po[-1]))
    assert _status(lambda: gm.run_with_mapping_states(rc, mp)) == _ffi.PHMM_EINVAL
    assert _status(lambda: out.mea(gm, rc, mp)) == _ffi.PHMM_EINVAL and out.untouched()


def test_the_weights_plane_counts_against_the_workspace_limit(gpu_lib, dbg):
    b, gm, rc, mp, po, nd = dbg
    out = _Prefilled(rc, int(po[-1]))
    _ffi.check(gpu_lib.phmm_set_workspace_limit(24 * int(po[-1]) - 8))
    try:
        assert _status(lambda: out.mea(gm, rc, mp)) == _ffi.PHMM_ECAPACITY and out.untouched()
    finally:
        _ffi.check(gpu_lib.phmm_set_workspace_limit(0))


# ------------------------------------------------------------------ 3. the caller contract of both entry points
@pytest.fixture(scope="module")
def ctx(gpu_lib):
    c = cc.Ctx()
    rng = np.random.default_rng(80)
    c.w = rng.normal(size=(c.entries, 3))
    c.ibw = rng.normal(size=c.bases)
    return c


@pytest.fixture(scope="module")
def scratch(gpu_lib):
    s = cc.DeviceArray(cc.SCRATCH_BYTES, 0)
    yield s
    s.free()


def _upload(a):
    d = cc.DeviceArray(a.nbytes, 0)
    assert cc.hip().hipMemcpy(d.p, a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == cc.HIP_SUCCESS
    return d


def _rows(ctx, device_inputs):
    L = _ffi_mea.lib()
    keep = [_upload(ctx.w), _upload(ctx.ibw)] if device_inputs else []
    pw, pib = (keep[0].p, keep[1].p) if device_inputs else (_P(ctx.w), _P(ctx.ibw))
    walk_outs = lambda c: [cc.Out("score", cc.F8, (c.R,)), cc.Out("path", cc.U4, (c.bases, c.stride)),  # noqa: E731
                           cc.Out("counts", cc.U4, (c.R, 4))]
    mea_outs = lambda c: [cc.Out("logp_forward", cc.F8, (c.R,))] + walk_outs(c) + [cc.Out("weights", cc.F8, (c.entries, 3))]  # noqa: E731
    sym = _ffi_mea.MEA_SYMBOLS["phmm_amd_mea.h"]
    walk = cc.Row("run_with_mapping_weighted_path", sym[:1], walk_outs,
                  lambda c, b: c.ffi.check(L.phmm_run_with_mapping_weighted_path(c.gm._h, c.rc._h, c.mp._h, pw, pib, b["score"],
                                                                                 b["path"], b["counts"])))
    mea = cc.Row("run_with_mapping_mea_path", sym[1:], mea_outs,
                 lambda c, b: c.ffi.check(L.phmm_run_with_mapping_mea_path(c.gm._h, c.rc._h, c.mp._h, 1.0, b["logp_forward"],
                                                                           b["score"], b["path"], b["counts"], b["weights"])))
    return {"walk": walk, "mea": mea}, keep


@pytest.mark.parametrize("which", ["walk", "mea"])
def test_device_pointers_and_a_busy_stream(ctx, scratch, which):
    """host inputs and outputs on the NULL stream are the reference; then device-pointer inputs and outputs into
    poisoned buffers, on the NULL stream and on a hipStreamNonBlocking stream that is still busy when the call starts:
    the same raw bits, and nothing behind an output's extent"""
    want = cc.run_host(ctx, _rows(ctx, False)[0][which])
    assert np.all(np.isfinite(want["score"]))
    rows, keep = _rows(ctx, True)
    row = rows[which]
    for stream in (None, cc.Stream()):
        d = cc.DeviceOutputs(ctx, row, stream)
        try:
            if stream is None:
                row.call(ctx, d.pointers())
                got, clean = d.read()
            else:
                with cc.on_stream(ctx.lib, stream):
                    cc.queue_work(stream, scratch)
                    d.poison(stream)
                    busy = stream.query()
                    row.call(ctx, d.pointers())
                    got, clean = d.read()
                assert busy == cc.HIP_ERROR_NOT_READY, "the queued work had drained before the call: the case ordered nothing"
            assert not cc.same_result(want, got), cc.same_result(want, got)
            assert clean, "bytes behind an output's extent were written"
        finally:
            d.free()
            if stream is not None:
                stream.destroy()
    for k in keep:
        k.free()


@pytest.mark.parametrize("which", ["walk", "mea"])
def test_four_calls_do_not_grow_the_workspace(ctx, which):
    row = _rows(ctx, False)[0][which]
    runs, ws = [], []
    for _ in range(4):
        runs.append(cc.run_host(ctx, row))
        ws.append(ctx.lib.phmm_workspace_bytes())
    assert ws[1] == ws[2] == ws[3], ws
    for k in (1, 2, 3):
        assert not cc.same_result(runs[0], runs[k]), (k, cc.same_result(runs[0], runs[k]))


# ------------------------------------------------------------------ 4. the MEA call
def _edges(arrays):
    return set(zip(arrays.edge_src.tolist(), arrays.edge_dst.tolist()))


def _is_a_walk(arrays, states):
    """path_states of a read: consecutive node states are joined by an edge (an Ins stays on its node)"""
    edges, prev = _edges(arrays), None
    for node, kind in states:
        if kind == "IB":
            assert prev is None
            continue
        if kind == "I":
            assert node == prev
        elif prev is not None:
            assert (prev, node) in edges, (prev, node, kind)
        prev = node
    return True


def _upper_bound(w, po, g0, g1, gaps):
    """per base the largest emitting weight, then n_max_gaps + 1 times the largest Del weight, added in path order: every
    addend is at least the path's at the same step (the weights are >= 0: a step the path leaves out adds >= 0), and a
    rounded addition is monotone in both arguments, so the bound holds without a tolerance"""
    total = 0.0
    for g in range(g0, g1):
        e = w[int(po[g]):int(po[g + 1])]
        total = total + (max(0.0, float(e[:, :2].max())) if len(e) else 0.0)  # (InsBegin: 0)
        for _ in range(gaps + 1):
            total = total + (float(e[:, 2].max()) if len(e) else 0.0)
    return total


def _mea_checks(arrays, reads, lists=None, del_weight=1.0, restate=True, what=""):
    gm, rc, mp, po, nd = _handles(arrays, reads, lists)
    off = rc.offsets.astype(np.int64)
    gaps = int(arrays.param.n_max_gaps)
    lf, score, path, counts, w = gm.run_with_mapping_mea_path(rc, mp, del_weight, want_weights=True)
    lf_s, sl, _ = gm.run_with_mapping_states(rc, mp, want_best=False)
    assert cc.same_bits(lf, lf_s)
    # the weights against numpy's exp of the states call's values
    with np.errstate(under="ignore"):
        want_w = np.exp(sl) * np.array([1.0, 1.0, del_weight])
    assert np.all(w[np.isneginf(sl)] == 0.0) and np.all(w >= 0.0)
    # A double below 2^-1022 is subnormal: its neighbours are 2^-1074 apart whatever its size, so "within 1 ulp" is an
    # absolute statement there and a relative bar of 2^-52 lies below the spacing.  The same reasoning (1 ulp each side,
    # the factor 2 on top) gives 4 * 2^-1074 for those values; every normal value keeps the relative bar.
    tiny = want_w < 2.0 ** -1022
    rel = float((np.abs(w - want_w) / np.where(tiny, 1.0, want_w))[~tiny].max(initial=0.0))
    sub = float(np.abs(w - want_w)[tiny].max(initial=0.0)) / 2.0 ** -1074
    print(f"{what}: weights within {rel / 2.0 ** -52:.2f} x 2^-52 of numpy.exp ({int((~tiny).sum())} normal values), within "
          f"{sub:.0f} x 2^-1074 ({int((tiny & (want_w > 0.0)).sum())} subnormal values), {int(np.isneginf(sl).sum())} exact zeros")
    assert rel <= EXP_BAR, rel
    assert sub <= 4.0, sub
    if del_weight == 0.0:
        assert np.all(w[:, 2] == 0.0)
    # the same bits from the weighted walk on those weights
    assert _same_bits(gm.run_with_mapping_weighted_path(rc, mp, w), (score, path, counts))
    # invariants
    bp_lp, bp_path, _ = gm.run_with_mapping_best_path(rc, mp)
    for j, r in enumerate(reads):
        ls = B.lists_of(po, nd, off[j], off[j + 1])
        e0, e1 = int(po[off[j]]), int(po[off[j + 1]])
        rows = path[off[j]:off[j + 1]]
        if restate:
            M.check_read(arrays, r, ls, w[e0:e1], None, float(score[j]), rows, counts[j].tolist())
        assert np.isfinite(score[j])  # (the states call accepted the read: it has a path)
        if bp_lp[j] > -np.inf:
            assert score[j] >= M.score_rows(arrays, r, ls, bp_path[off[j]:off[j + 1]], w[e0:e1])[0], j
        assert score[j] <= _upper_bound(w, po, off[j], off[j + 1], gaps), j
        assert counts[j].tolist() == M.counts_of(arrays, r, ls, rows)
        assert M.score_rows(arrays, r, ls, rows, w[e0:e1])[0] == score[j]
        assert _is_a_walk(arrays, D.path_states(mp, j, path))
    return gm, rc, mp, score, path, counts


def test_mea_linear_mock(gpu_lib):
    a = B.linear(0.01)
    reads = [b"ATTCGTCGT", b"ATTCGCATCGT", b"ATTCGATGGT"]
    gm, rc, mp, score, path, counts = _mea_checks(a, reads, what="linear mock")
    # the posterior sits on the true alignments: one deletion, one insertion, one substitution
    assert D.path_states(mp, 0, path) == [(v, "M") for v in range(5)] + [(5, "D")] + [(v, "M") for v in range(6, 10)]
    assert counts.tolist() == [[9, 0, 0, 1], [10, 0, 1, 0], [9, 1, 0, 0]]
    print("expected shared states", score.tolist(), "of", counts.sum(axis=1).tolist())
    _, s0, p0, c0, w0 = gm.run_with_mapping_mea_path(rc, mp, 0.0, want_weights=True)
    assert np.all(w0[:, 2] == 0.0) and np.all(s0 <= [len(r) for r in reads])


@pytest.mark.parametrize("graph", ["zoo", "dbg"])
@pytest.mark.parametrize("del_weight", [1.0, 0.0, 0.5])
def test_mea_small_graphs(gpu_lib, graph, del_weight):
    b = base_case(graph)
    _mea_checks(b["arrays"], b["reads"], del_weight=del_weight, restate=del_weight == 1.0, what=f"{graph}, del_weight {del_weight}")


@pytest.mark.parametrize("which", range(6))
def test_mea_fuzz(gpu_lib, which):
    c = B.fuzz_cases()[which]
    _mea_checks(c["arrays"], c["reads"], restate=False, what=c["tag"])


@pytest.mark.parametrize("gaps", [0, 4, 6])
def test_mea_del_levels(gpu_lib, gaps):
    arrays, read = B.two_deletions()
    _mea_checks(with_gaps(arrays, gaps), [read], restate=False, what=f"n_max_gaps = {gaps}")


@pytest.mark.parametrize("width", (64, 129, 400))
def test_mea_list_widths(gpu_lib, width):
    arrays, reads = B.width_reads(width)
    po0, nd0 = _gpu_lists(arrays, reads)
    _mea_checks(arrays, reads, B.pad_lists(po0, nd0, reads, arrays.n_nodes, width), restate=False, what=f"lists padded to {width}")


def _states_call_takes(bp, lists):
    """the reads the states call accepts: probability > 0 on their lists and no node twice in a list"""
    return [j for j in range(len(lists)) if bp[j] > -np.inf and all(len(set(x)) == len(x) for x in lists[j])]


def test_mea_many_short_reads_and_odd_lists(gpu_lib):
    """the reads of the odd fixtures that the states call accepts: it refuses a set with a read of probability 0 on its
    lists or with a node twice in a list, and so does the MEA call (the weighted walk takes both)"""
    arrays, reads, lists = B.many_short_reads()
    gm, rc, mp, po, nd = _handles(arrays, reads, B.csr(lists))
    out = _Prefilled(rc, int(po[-1]))
    assert _status(lambda: gm.run_with_mapping_states(rc, mp)) == _status(lambda: out.mea(gm, rc, mp)) == _ffi.PHMM_EINVAL
    assert out.untouched()
    keep = _states_call_takes(gm.run_with_mapping_best_path(rc, mp, want_path=False)[0], lists)
    assert len(keep) > 128
    _mea_checks(arrays, [reads[j] for j in keep], B.csr([lists[j] for j in keep]), restate=False, what="short reads")
    n = 0
    for g in B.odd_cases("ord"):
        gm, rc, mp, po, nd = _handles(g["arrays"], g["reads"], B.csr(g["lists"]))
        keep = _states_call_takes(gm.run_with_mapping_best_path(rc, mp, want_path=False)[0], g["lists"])
        if keep:
            _mea_checks(g["arrays"], [g["reads"][j] for j in keep], B.csr([g["lists"][j] for j in keep]), what=g["tag"])
            n += len(keep)
    assert n > 50


def test_mea_long_read(gpu_lib):
    arrays, read = B.long_read()
    _mea_checks(arrays, [read], restate=False, what="one read of 3000 bases")


def test_mea_chunks(gpu_lib, dbg):
    """the weights plane of the whole call and the walk's fixed arrays, then records and rows of two reads: the same bits"""
    b, gm, rc, mp, po, nd = dbg
    off = rc.offsets.astype(np.int64)
    want = gm.run_with_mapping_mea_path(rc, mp, want_weights=True)
    stride = want[2].shape[1]
    per_read = [16 * (int(po[off[j + 1]]) - int(po[off[j]])) + 4 * stride * int(off[j + 1] - off[j]) for j in range(len(rc))]
    assert 2 * max(per_read) < sum(per_read) / 2
    _ffi.check(gpu_lib.phmm_set_workspace_limit(24 * int(po[-1]) + 2 * max(per_read) + (64 << 10)))
    try:
        got = gm.run_with_mapping_mea_path(rc, mp, want_weights=True)
        launches = _ffi.last_call_stats(STATS_HINTED)[1]
    finally:
        _ffi.check(gpu_lib.phmm_set_workspace_limit(0))
    assert launches >= 4 and _same_bits(got, want)


# ------------------------------------------------------------------ 5. relabelling
@pytest.mark.parametrize("ordering", ORDERINGS)
@pytest.mark.parametrize("graph", ["dbg", "zoo"])
def test_relabelling(gpu_lib, graph, ordering):
    """other node ids and another edge order, the lists carried onto the new ids in the same slot order and the weights
    with their entries: ranks go by slot and an edge permutation only reorders candidates of equal rank, so every output
    keeps its bits"""
    b = base_case(graph)
    gm, rc, mp, po, nd = _handles(b["arrays"], b["reads"])
    w, ib, _ = _mixed(90, ORDERINGS.index(ordering), rc, po, with_ib=True)
    want = gm.run_with_mapping_weighted_path(rc, mp, w, ib)
    case = relabelled_case(graph, ordering)
    po2, nd2, _ = carry_mappings((po, nd, None), case["node_perm"])
    gm2, rc2, mp2, _, _ = _handles(case["arrays"], b["reads"], (po2, nd2))
    got = gm2.run_with_mapping_weighted_path(rc2, mp2, w, ib)  # (entry a of the carried lists is entry a: the same weights)
    assert _same_bits(want, got)
    off = rc.offsets.astype(np.int64)
    for j in (0, 7):  # (and against the restatement on the new labels)
        e0, e1 = int(po[off[j]]), int(po[off[j + 1]])
        M.check_read(case["arrays"], b["reads"][j], B.lists_of(po2, nd2, off[j], off[j + 1]), w[e0:e1], ib[off[j]:off[j + 1]],
                     float(got[0][j]), got[1][off[j]:off[j + 1]], got[2][j].tolist())
