"""GPU: alignment records -- the CIGAR and the node walk of the best path or of S sampled paths of every read over its
mapping lists (phmm_run_with_mapping_alignments, PHMMModel.run_with_mapping_alignments, include/phmm_amd_align.h).

Tier 1 holds the records word for word to compress() of tests/alignments_ref.py over the rows of the Python
restatements of the two parent calls (best_path_ref, sample_paths_ref), which are not the code under test.  out_logp of
the best path is the restatement's double; out_counts is what score_path counts on the restatement's rows; for samples
out_logp, out_path_logp and out_counts carry the bits phmm_run_with_mapping_sample_paths returns for the same
arguments, which tests/test_gpu_sample_paths.py pins to the restatement.
Tier 2 runs shapes the restatements are too slow for: the parent's entry points with a host out_path on the same
model, reads and lists, and the records must equal compress() of the rows they return.
The contract part feeds the call the way callers do: device outputs behind poison, a busy stream, repeated calls, NULL
outputs, a model that changes under the handle, refusals.  Every alignment of every test passes the header's three
invariants (alignments_ref.check_invariants) and reads back as the states path_states gives for the rows.

Nothing here has a tolerance: every comparison is on integers or raw bits."""
import ctypes as C

import numpy as np
import pytest

import dbgphmm_amd as D
import alignments_ref as A
import best_path_ref as B
import caller_cases as cc
import sample_paths_ref as S
from dbgphmm_amd import _ffi, _ffi_align
from graph_cases import ORDERINGS, base_case, carry_mappings, relabelled_case, with_gaps

pytestmark = pytest.mark.gpu
STATS_HINTED = 2
SENTINEL = 0xDEAD0


def _bits(x, y):
    x, y = np.asarray(x), np.asarray(y)
    return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


def _handles(reads, lists):
    rc = D.ReadCollection(reads)
    po, nd = B.csr(lists)
    return rc, D.Mappings.from_arrays(rc, po, nd)


def _lists(rc, mp):
    po, nd, _ = mp.arrays()
    off = rc.offsets.astype(np.int64)
    return [B.lists_of(po, nd, off[j], off[j + 1]) for j in range(len(rc))]


def _alignments(gm, rc, mp, n_samples=0, seed=0):
    lp, plp, counts, al = gm.run_with_mapping_alignments(rc, mp, n_samples, seed)
    planes = max(n_samples, 1)
    assert lp.shape == (len(rc),) and counts.shape == (len(rc), planes, 4) and len(al) == len(rc) * planes
    assert (plp is None) if n_samples == 0 else plp.shape == (len(rc), n_samples)
    return lp, plp, counts, al


def _hold(arrays, reads, lists, al, counts, rows_of, what):
    """every alignment a = r * S' + s: the record is compress(rows_of(r, s)) word for word, passes the invariants against
    out_counts, and reads back (dbgphmm_amd.Alignments.states) as the states the rows spell -> the records"""
    arr = al.arrays()
    op_off, ops, run_off, rn, rl = arr
    planes = max(al.n_samples, 1)
    assert op_off.dtype == run_off.dtype == np.uint64 and ops.dtype == rn.dtype == rl.dtype == np.uint32
    assert op_off[0] == 0 and run_off[0] == 0 and int(op_off[-1]) == ops.size and int(run_off[-1]) == rn.size == rl.size
    assert np.all(np.diff(op_off.astype(np.int64)) >= 0) and np.all(np.diff(run_off.astype(np.int64)) >= 0)
    recs = []
    for r, read in enumerate(reads):
        for s in range(planes):
            a = al.index(r, s)
            rec = A.records_of(arr, a)
            rows = rows_of(r, s)
            want = A.compress(arrays, read, lists[r], rows)
            assert rec == want, (what, r, s, A.cigar_string(rec[0]), A.cigar_string(want[0]), rec[1:], want[1:])
            A.check_invariants(*rec, len(read), counts[r, s].tolist())
            assert al.states(a) == A.states_of_rows(lists[r], rows) == A.expand(*rec), (what, r, s)
            recs.append(rec)
    return recs


def _against_parent(gm, arrays, reads, rc, mp, n_samples, seed, what):
    """the parent's call with a host out_path, then the new call on the same handles: the scores and counts carry the
    parent's bits and the records are compress() of the parent's rows -> (lists, parent rows, Alignments, records)"""
    off = rc.offsets.astype(np.int64)
    lists = _lists(rc, mp)
    if n_samples == 0:
        lp0, path, c0 = gm.run_with_mapping_best_path(rc, mp)
        plp0, c0 = None, c0[:, None, :]
        rows_of = lambda r, s: path[off[r]:off[r + 1]]  # noqa: E731
    else:
        lp0, plp0, path, c0, _ = gm.run_with_mapping_sample_paths(rc, mp, n_samples, seed)
        rows_of = lambda r, s: path[s, off[r]:off[r + 1]]  # noqa: E731
    lp, plp, counts, al = _alignments(gm, rc, mp, n_samples, seed)
    assert _bits(lp, lp0) and _bits(counts, c0) and (n_samples == 0 or _bits(plp, plp0)), what
    recs = _hold(arrays, reads, lists, al, counts, rows_of, what)
    return lists, path, al, recs


def _same_records(x, y):
    return all(_bits(a, b) for a, b in zip(x.arrays(), y.arrays()))


# ------------------------------------------------------------------ tier 1: best path against best_path_ref
def _best_against_ref(arrays, reads, lists, what):
    gm = D.PHMMModel(arrays)
    rc, mp = _handles(reads, lists)
    lp, plp, counts, al = _alignments(gm, rc, mp)
    ref = [B.best_path_ref(arrays, r, ls) for r, ls in zip(reads, lists)]
    for j, (best, rows) in enumerate(ref):
        assert lp[j] == best, (what, j, lp[j], best)
        want = B.score_path(arrays, reads[j], lists[j], rows)[2] if best > -np.inf else [0, 0, 0, 0]
        assert counts[j, 0].tolist() == want, (what, j)
    recs = _hold(arrays, reads, lists, al, counts, lambda r, s: ref[r][1], what)
    return gm, rc, mp, al, recs


@pytest.mark.parametrize("logs", ["integer", "ordinary"])
@pytest.mark.parametrize("graph", ["dbg", "zoo"])
def test_best_path_records_small_graphs(gpu_lib, graph, logs):
    """12 reads of at most 40 bases each"""
    c = B.int_case(graph) if logs == "integer" else S.graph_fixture(graph)
    assert len(c["reads"]) == 12 and max(len(r) for r in c["reads"]) <= 40
    _, _, _, al, recs = _best_against_ref(c["arrays"], c["reads"], c["lists"], f"{logs}-log {graph}")
    assert any(rec[0] for rec in recs)


@pytest.mark.parametrize("flavour", ["ord", "int"])
def test_best_path_records_odd_lists(gpu_lib, flavour):
    n = with_path = 0
    for g in B.odd_cases(flavour):
        _, _, _, al, recs = _best_against_ref(g["arrays"], g["reads"], g["lists"], g["tag"])
        n, with_path = n + len(recs), with_path + sum(1 for rec in recs if rec[0])
        if g["tag"].endswith("forms, p_mismatch = -inf, init on node 2"):
            j = g["reads"].index(b"AATT")  # InsBegin twice, a Del behind it, then two matches
            assert al.cigar_string(j) == "2I1D2=" and al.walk(j) == [(2, 3)]
            assert al.states(j) == [(None, "IB"), (None, "IB"), (2, "D"), (3, "M"), (4, "M")]
    assert n == 213 and 0 < with_path < n


def test_best_path_records_bubble_and_two_deletions(gpu_lib):
    arrays, read, orders = B.bubble_case()
    for name, (order, nodes) in orders.items():
        _, _, _, al, _ = _best_against_ref(arrays, [read], [[order] * len(read)], f"bubble, {name}")
        assert al.cigar_string(0) == "5=" and al.nodes(0) == nodes
    arrays, read = B.two_deletions()
    for gaps in (0, 4, 6):
        a = with_gaps(arrays, gaps)
        gm, rc = D.PHMMModel(a), D.ReadCollection([read])
        mp = gm.generate_mappings(rc, None, True)[0]
        _, _, _, al, _ = _best_against_ref(a, [read], _lists(rc, mp), f"two deletions, n_max_gaps = {gaps}")
        cigar = al.cigar(0)
        if gaps:  # the two Dels stand in one row: one CIGAR run of 2
            assert sum(n for n, op in cigar if op == A.DEL) == 2 and (2, A.DEL) in cigar
        else:     # one Del per row at most, and an emitting state between two rows' Dels
            assert all(n == 1 for n, op in cigar if op == A.DEL)


# ------------------------------------------------------------------ tier 1: samples against sample_paths_ref
def _samples_against_ref(k):
    f = S.fixtures()[k]
    arrays, reads, lists, n, seed = f["arrays"], f["reads"], f["lists"], f["n_samples"], f["seed"]
    want = S.fixture_samples(k)
    gm = D.PHMMModel(arrays)
    rc, mp = _handles(reads, lists)
    lp, plp, counts, al = _alignments(gm, rc, mp, n, seed)
    lp0, plp0, _, c0, _ = gm.run_with_mapping_sample_paths(rc, mp, n, seed, want_path=False)
    assert _bits(lp, lp0) and _bits(plp, plp0) and _bits(counts, c0), f["tag"]
    for j in range(len(reads)):
        assert (lp[j] == -np.inf) == (want[j]["logz"] == -np.inf)
        assert np.array_equal(counts[j], want[j]["counts"]), (f["tag"], j)
    return _hold(arrays, reads, lists, al, counts, lambda r, s: want[r]["rows"][s], f["tag"])


@pytest.mark.parametrize("k", [0, 1], ids=["dbg", "zoo"])
def test_sample_records_small_graphs(gpu_lib, k):
    """S = 64 on dbg and zoo"""
    assert S.fixtures()[k]["n_samples"] == 64
    recs = _samples_against_ref(k)
    assert len(recs) == 12 * 64 and len({repr(r) for r in recs}) > 12  # (the samples of a read differ)


def test_sample_records_odd_lists(gpu_lib):
    """S = 3 on every odd-list group"""
    fx = S.fixtures()
    n = 0
    for k in range(3, len(fx)):
        assert fx[k]["n_samples"] == 3
        n += len(_samples_against_ref(k))
    assert n == 3 * 213


# ------------------------------------------------------------------ tier 2: against the parent's rows
@pytest.fixture(scope="module")
def long_run(gpu_lib):
    arrays, read = B.long_read()
    reads = [read[:n] for n in (1, 63, 64, 65, 127, 128, 129, 3000)]
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    mp = gm.generate_mappings(rc, None, True)[0]
    return arrays, reads, gm, rc, mp


@pytest.mark.parametrize("n_samples", [0, 2])
def test_tile_seams(long_run, n_samples):
    """reads that end one base before, on and behind a tile of 64 bases, and one of 3000 whose runs span many tiles"""
    arrays, reads, gm, rc, mp = long_run
    _, _, al, recs = _against_parent(gm, arrays, reads, rc, mp, n_samples, 5, f"tile seams, S = {n_samples}")
    planes = max(n_samples, 1)
    for s in range(planes):
        cigar, _, run_len = recs[7 * planes + s]
        longest_eq = max(w >> 4 for w in cigar if w & 15 == A.EQ)
        print(f"3000 bases, plane {s}: {len(cigar)} CIGAR words, longest = run {longest_eq}; {len(run_len)} walk runs, "
              f"longest {max(run_len)}")
        if n_samples == 0:
            assert longest_eq > 64 and max(run_len) > 64  # (the case covers a run across a seam)
    assert recs[0][0] and len(recs[0][0]) == 1  # the read of one base


@pytest.fixture(scope="module")
def dbg_base(gpu_lib):
    b = base_case("dbg")
    gm, rc = D.PHMMModel(b["arrays"]), D.ReadCollection(b["reads"])
    mp = gm.generate_mappings(rc, None, True)[0]
    return b, gm, rc, mp


@pytest.mark.parametrize("ordering", ORDERINGS)
def test_relabelling(dbg_base, ordering):
    """the lists carried onto other node ids: the CIGARs keep their bits, the walks follow the ids"""
    b, gm, rc, mp = dbg_base
    po, nd, _ = mp.arrays()
    case = relabelled_case("dbg", ordering)
    po2, nd2, _ = carry_mappings((po, nd, None), case["node_perm"])
    gm2, rc2 = D.PHMMModel(case["arrays"]), D.ReadCollection(b["reads"])
    mp2 = D.Mappings.from_arrays(rc2, po2, nd2)
    base_al = _alignments(gm, rc, mp)[3]
    for n_samples in (0, 2):
        _, _, al, recs = _against_parent(gm2, case["arrays"], b["reads"], rc2, mp2, n_samples, 9, f"dbg {ordering}, S = {n_samples}")
        lens = [n for _, _, rl in recs for n in rl]
        if ordering == "reverse":
            assert lens and max(lens) == 1  # the successor on a unitig is id - 1: no run
        if ordering == "identity":
            assert max(lens) > 1
        if n_samples == 0:
            assert _bits(al.arrays()[0], base_al.arrays()[0]) and _bits(al.arrays()[1], base_al.arrays()[1])
            perm = case["node_perm"]
            for a in range(len(al)):
                assert al.nodes(a) == [int(perm[v]) for v in base_al.nodes(a)]


@pytest.mark.parametrize("n_samples", [0, 3])
def test_wide_lists_interleaved(gpu_lib, n_samples):
    """lists padded in front to 65, 129 and 400 with unreachable nodes, so that chosen slots pass 255 and the 400 class
    runs, narrow and wide reads interleaved in one call"""
    c = B.int_case("zoo")
    widths = (0, 65, 129, 400)
    lists = [ls if j % 4 == 0 else B.pad_unreachable(ls, c["n_real"], widths[j % 4], front=True) for j, ls in enumerate(c["lists"])]
    gm = D.PHMMModel(c["arrays"])
    rc, mp = _handles(c["reads"], lists)
    _, path, al, recs = _against_parent(gm, c["arrays"], c["reads"], rc, mp, n_samples, 3, f"wide lists, S = {n_samples}")
    assert _ffi.last_call_stats(STATS_HINTED)[1] >= 5  # both capacity classes, the walk, the count and the write pass
    slots = path[(path != A.NONE) & (path != A.INS_BEGIN)] >> 2
    assert int(slots.max()) > 255
    # the padding changes no record: the same reads on their own lists
    rc0, mp0 = _handles(c["reads"], c["lists"])
    assert _same_records(al, _alignments(gm, rc0, mp0, n_samples, 3)[3])


def _fixed_bytes(arrays, R, n_samples):
    """the control arrays of the parent call, each at a multiple of 256, and the model's init and trans"""
    if n_samples == 0:
        sizes = (8 * R, 8 * (R + 1), 4 * R, 4 * R, 4 * R, 16 * R)
    else:
        sizes = (8 * R, 8 * (R + 1), 8 * R, 8 * R, 4 * R, 4 * R, 8 * R * n_samples, 16 * R * n_samples)
    fixed = 0
    for nbytes in sizes:
        fixed = (fixed + 255) // 256 * 256 + nbytes
    return fixed + 8 * (arrays.n_nodes + arrays.n_edges)


@pytest.mark.parametrize("n_samples", [0, 3])
def test_many_short_reads_in_chunks(gpu_lib, n_samples):
    """320 reads, unlimited and then in four chunks or so under a workspace limit: the same bits"""
    arrays, reads, lists = B.many_short_reads()
    gm = D.PHMMModel(arrays)
    rc, mp = _handles(reads, lists)
    _, _, al, recs = _against_parent(gm, arrays, reads, rc, mp, n_samples, 31, f"many short reads, S = {n_samples}")
    lp, plp, counts, _ = _alignments(gm, rc, mp, n_samples, 31)
    assert _ffi.last_call_stats(STATS_HINTED)[1] == 4  # one forward class, the walk, the count and the write pass
    assert len(recs) == 320 * max(n_samples, 1) and any(rec[0] for rec in recs)
    stride, planes = arrays.param.n_max_gaps + 2, max(n_samples, 1)
    if n_samples == 0:
        per_read = [16 * sum(len(x) for x in ls) + 4 * stride * len(r) for r, ls in zip(reads, lists)]
    else:
        per_read = [128 * sum(len(x) for x in ls) + 8 * len(r) + 4 * stride * planes * len(r) for r, ls in zip(reads, lists)]
    _ffi.check(gpu_lib.phmm_set_workspace_limit(_fixed_bytes(arrays, len(reads), n_samples) + sum(per_read) // 4))
    try:
        lp2, plp2, counts2, al2 = _alignments(gm, rc, mp, n_samples, 31)
        launches = _ffi.last_call_stats(STATS_HINTED)[1]
    finally:
        _ffi.check(gpu_lib.phmm_set_workspace_limit(0))
    assert launches >= 12 and launches % 4 == 0, launches  # three chunks or more, so chunks start behind read 0
    assert _bits(lp, lp2) and _bits(counts, counts2) and (n_samples == 0 or _bits(plp, plp2))
    assert _same_records(al, al2)


def test_one_sample_is_sample_0_of_64_and_a_read_alone(dbg_base):
    b, gm, rc, mp = dbg_base
    lp64, plp64, c64, al64 = _alignments(gm, rc, mp, 64, 17)
    lp1, plp1, c1, al1 = _alignments(gm, rc, mp, 1, 17)
    assert _bits(lp1, lp64) and _bits(plp1[:, 0], plp64[:, 0]) and _bits(c1[:, 0], c64[:, 0])
    for r in range(len(rc)):
        assert A.records_of(al1.arrays(), r) == A.records_of(al64.arrays(), al64.index(r, 0))
    # a read alone at index 0 has the bits it gets as read 0 of the set rotated to start with it (the random stream goes by
    # the read's index); the best path does not depend on the index at all
    po, nd, _ = mp.arrays()
    off = rc.offsets.astype(np.int64)
    lists = _lists(rc, mp)
    lp0, _, c0, al0 = _alignments(gm, rc, mp)
    for j in (0, 5, len(rc) - 1):
        rc1, mp1 = _handles([b["reads"][j]], [lists[j]])
        lpa, _, ca, ala = _alignments(gm, rc1, mp1)
        assert lpa[0] == lp0[j] and _bits(ca[0], c0[j]) and A.records_of(ala.arrays(), 0) == A.records_of(al0.arrays(), j)
        rot_r, rot_l = b["reads"][j:] + b["reads"][:j], lists[j:] + lists[:j]
        rc2, mp2 = _handles(rot_r, rot_l)
        lpb, plpb, cb, alb = _alignments(gm, rc2, mp2, 4, 17)
        lpc, plpc, cc_, alc = _alignments(gm, rc1, mp1, 4, 17)
        assert lpb[0] == lpc[0] and _bits(plpb[0], plpc[0]) and _bits(cb[0], cc_[0])
        for s in range(4):
            assert A.records_of(alb.arrays(), s) == A.records_of(alc.arrays(), s)


# ------------------------------------------------------------------ the contract
@pytest.fixture(scope="module")
def ctx(gpu_lib):
    return cc.Ctx()


@pytest.fixture(scope="module")
def scratch(gpu_lib):
    s = cc.DeviceArray(cc.SCRATCH_BYTES, 0)
    yield s
    s.free()


def _row(ctx, n_samples):
    """the new entry points as a row of caller_cases: the call, the export into the caller's buffers, the destroy"""
    AL = _ffi_align.lib()
    planes = max(n_samples, 1)
    h = C.c_void_p()
    _ffi.check(AL.phmm_run_with_mapping_alignments(ctx.gm._h, ctx.rc._h, ctx.mp._h, n_samples, 77, None, None, None, C.byref(h)))
    n_ops, n_runs = int(AL.phmm_alignments_total_ops(h)), int(AL.phmm_alignments_total_runs(h))
    assert AL.phmm_alignments_count(h) == ctx.R * planes and n_ops >= ctx.R and n_runs >= 1
    AL.phmm_alignments_destroy(h)
    A_ = ctx.R * planes
    outs = [cc.Out("logp", cc.F8, (ctx.R,)), cc.Out("counts", cc.U4, (ctx.R, planes, 4)), cc.Out("op_off", cc.U8, (A_ + 1,)),
            cc.Out("ops", cc.U4, (n_ops,)), cc.Out("run_off", cc.U8, (A_ + 1,)), cc.Out("run_node", cc.U4, (n_runs,)),
            cc.Out("run_len", cc.U4, (n_runs,))]
    if n_samples:
        outs.append(cc.Out("path_logp", cc.F8, (ctx.R, n_samples)))

    def call(c, b):
        h = C.c_void_p()
        c.ffi.check(AL.phmm_run_with_mapping_alignments(c.gm._h, c.rc._h, c.mp._h, n_samples, 77, b["logp"], b.get("path_logp"),
                                                        b["counts"], C.byref(h)))
        try:
            c.ffi.check(AL.phmm_alignments_export(h, b["op_off"], b["ops"], b["run_off"], b["run_node"], b["run_len"]))
        finally:
            AL.phmm_alignments_destroy(h)
    return cc.Row(f"run_with_mapping_alignments_{n_samples}", list(_ffi_align.ALIGN_SYMBOLS["phmm_amd_align.h"]),
                  lambda c: outs, call)


@pytest.mark.parametrize("n_samples", [0, 3])
def test_device_outputs_and_a_busy_stream(ctx, scratch, n_samples):
    """every output, the exported arrays included, into poisoned device buffers: the host form's bits and nothing behind
    an output's extent; then the same on a hipStreamNonBlocking stream that is still busy when the call starts"""
    row = _row(ctx, n_samples)
    want = cc.run_host(ctx, row)
    # the host form itself against the parent's rows
    arr = tuple(want[k] for k in ("op_off", "ops", "run_off", "run_node", "run_len"))
    al = D.Alignments.from_arrays(ctx.R, n_samples, *arr)
    off = ctx.rc.offsets.astype(np.int64)
    lists = _lists(ctx.rc, ctx.mp)
    if n_samples == 0:
        _, path, _ = ctx.gm.run_with_mapping_best_path(ctx.rc, ctx.mp)
        rows_of = lambda r, s: path[off[r]:off[r + 1]]  # noqa: E731
    else:
        _, _, path, _, _ = ctx.gm.run_with_mapping_sample_paths(ctx.rc, ctx.mp, n_samples, 77)
        rows_of = lambda r, s: path[s, off[r]:off[r + 1]]  # noqa: E731
    _hold(ctx.arrays, ctx.reads, lists, al, want["counts"], rows_of, f"caller fixture, S = {n_samples}")
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


@pytest.mark.parametrize("chunked", [False, True])
@pytest.mark.parametrize("n_samples", [0, 3])
def test_four_calls_do_not_grow_the_workspace(ctx, n_samples, chunked):
    """each call's handle is destroyed before the next call: the workspace is the same after calls 2, 3 and 4 and every
    call returns the same bits; unlimited, and in chunks (where the handle's arrays grow chunk by chunk)"""
    row = _row(ctx, n_samples)
    if chunked:  # a third of what the call stages and records, beside its fixed arrays: three chunks or more
        planes = max(n_samples, 1)
        total = (128 * ctx.entries + 8 * ctx.bases if n_samples else 16 * ctx.entries) + 4 * ctx.stride * planes * ctx.bases
        _ffi.check(ctx.lib.phmm_set_workspace_limit(_fixed_bytes(ctx.arrays, ctx.R, n_samples) + total // 3))
    try:
        runs, ws = [], []
        for _ in range(4):
            runs.append(cc.run_host(ctx, row))
            ws.append(ctx.lib.phmm_workspace_bytes())
            launches = _ffi.last_call_stats(STATS_HINTED)[1]
    finally:
        _ffi.check(ctx.lib.phmm_set_workspace_limit(0))
    assert ws[1] == ws[2] == ws[3], ws
    for k in (1, 2, 3):
        assert not cc.same_result(runs[0], runs[k]), (k, cc.same_result(runs[0], runs[k]))
    if chunked:
        assert launches >= 8, launches  # two chunks or more
        assert not cc.same_result(cc.run_host(ctx, row), runs[0])  # the unlimited call's bits


def test_out_null_gives_scores_and_counts(ctx):
    AL = _ffi_align.lib()
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for n_samples in (0, 3):
        lp, plp, counts, al = _alignments(ctx.gm, ctx.rc, ctx.mp, n_samples, 77)
        lp2, plp2, counts2 = np.full_like(lp, 7.5), np.full((ctx.R, max(n_samples, 1)), 7.5), np.full_like(counts, 77)
        _ffi.check(AL.phmm_run_with_mapping_alignments(ctx.gm._h, ctx.rc._h, ctx.mp._h, n_samples, 77, P(lp2), P(plp2), P(counts2), None))
        assert _ffi.last_call_stats(STATS_HINTED)[1] in (2, 3)  # the parent's launches: no staged rows, no compaction
        assert _bits(lp, lp2) and _bits(counts, counts2)
        assert _bits(plp, plp2) if n_samples else np.all(plp2 == 7.5)  # (the best path writes no out_path_logp)
        _ffi.check(AL.phmm_run_with_mapping_alignments(ctx.gm._h, ctx.rc._h, ctx.mp._h, n_samples, 77, None, None, None, None))
    # no reads: no output array is written and the handle holds 0 alignments
    rc0 = D.ReadCollection([])
    mp0 = D.Mappings.from_arrays(rc0, np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint32))
    out = np.full(4, 7.5)
    h = C.c_void_p()
    _ffi.check(AL.phmm_run_with_mapping_alignments(ctx.gm._h, rc0._h, mp0._h, 0, 1, P(out), P(out), None, C.byref(h)))
    offs = np.full(2, 9, dtype=np.uint64)
    assert np.all(out == 7.5) and h.value and AL.phmm_alignments_count(h) == 0
    _ffi.check(AL.phmm_alignments_export(h, P(offs[:1]), None, P(offs[1:]), None, None))
    AL.phmm_alignments_destroy(h)
    assert offs.tolist() == [0, 0]


def test_same_handle_new_numbers(gpu_lib):
    """after phmm_model_set_probs and phmm_model_set_params (n_max_gaps 2 -> 0, rows of 4 words -> rows of 2) the call
    follows the handle's current numbers: the records of a fresh model, and compress() of the parent's rows"""
    g = [g for g in B.odd_cases("ord") if g["tag"].endswith("list oddities, n_max_gaps = 2")][0]
    a1, reads, lists = g["arrays"], g["reads"], g["lists"]
    a3 = B.odd_arrays("int", 0)
    a2 = D.PHMMArrays(a1.param, a1.emission, a3.init_logp, a1.edge_src, a1.edge_dst, a3.trans_logp)
    gm = D.PHMMModel(a1)
    rc, mp = _handles(reads, lists)
    first = _alignments(gm, rc, mp)[0]
    gm.set_probs(a2.init_logp, a2.trans_logp)
    for n_samples in (0, 3):
        _, _, al, _ = _against_parent(gm, a2, reads, rc, mp, n_samples, 21, "after set_probs")
        assert _same_records(al, _alignments(D.PHMMModel(a2), rc, mp, n_samples, 21)[3])
    assert not np.array_equal(_alignments(gm, rc, mp)[0], first)
    cp = a3.param.to_c()
    _ffi.check(_ffi.lib().phmm_model_set_params(gm._h, C.byref(cp)))
    gm.param = a3.param  # (PHMMModel sizes the parent's rows by its param)
    for n_samples in (0, 3):
        _, path, al, _ = _against_parent(gm, a3, reads, rc, mp, n_samples, 21, "after set_params, n_max_gaps 2 -> 0")
        assert path.shape[-1] == 2
        assert _same_records(al, _alignments(D.PHMMModel(a3), rc, mp, n_samples, 21)[3])


def _status(f):
    try:
        f()
    except _ffi.PhmmError as e:
        return e.code
    return _ffi.PHMM_OK


def test_refusals_leave_everything_as_it_was(dbg_base):
    b, gm, rc, mp = dbg_base
    AL = _ffi_align.lib()
    po, nd, _ = mp.arrays()
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    R = len(rc)
    lp, plp, counts = np.full(R, 7.5), np.full((R, 64), 7.5), np.full((R, 64, 4), 77, dtype=np.uint32)
    h = C.c_void_p(SENTINEL)

    def call(rc_, mp_, n_samples):
        _ffi.check(AL.phmm_run_with_mapping_alignments(gm._h, rc_._h, mp_._h, n_samples, 1, P(lp), P(plp), P(counts), C.byref(h)))

    def untouched():
        return h.value == SENTINEL and bool(np.all(lp == 7.5) and np.all(plp == 7.5) and np.all(counts == 77))
    n = rc.total_bases()

    def over():  # (a list of 401 is refused where the lists are handed over)
        call(rc, D.Mappings.from_arrays(rc, np.arange(n + 1, dtype=np.uint64) * 401, np.tile(np.arange(401, dtype=np.uint32), n)), 0)
    assert _status(over) == _ffi.PHMM_ECAPACITY and untouched()
    bad = nd.copy()
    bad[len(bad) // 2] = b["arrays"].n_nodes
    for n_samples in (0, 2):
        assert _status(lambda: call(rc, D.Mappings.from_arrays(rc, po, bad), n_samples)) == _ffi.PHMM_EINVAL and untouched()
    assert _status(lambda: call(rc, mp, 65)) == _ffi.PHMM_EINVAL and untouched()
    rc2 = D.ReadCollection(b["reads"][:2])
    for n_samples in (0, 2):
        assert _status(lambda: call(rc2, mp, n_samples)) == _ffi.PHMM_EINVAL and untouched()
    for hs in ((None, rc._h, mp._h), (gm._h, None, mp._h), (gm._h, rc._h, None)):
        assert AL.phmm_run_with_mapping_alignments(*hs, 0, 1, P(lp), P(plp), P(counts), C.byref(h)) == _ffi.PHMM_EINVAL
    assert untouched()
    call(rc, mp, 64)  # and the same buffers take a good call
    assert h.value != SENTINEL and not np.any(lp == 7.5) and AL.phmm_alignments_count(h) == R * 64
    AL.phmm_alignments_destroy(h)
