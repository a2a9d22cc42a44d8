"""The compute entry points of the C ABI as a table, for the tests of HOW they are called (test_gpu_caller_contract.py):
on a caller's stream, into device buffers, many times in a row.

Every row runs one entry point -- or the shortest chain that shows it: a likelihood handle is made, moved and read in
one row -- through the raw ABI (`_ffi.lib()`, handles via `._h`) on the shared small fixture and names its outputs.  The
caller of a row decides where each output lives (host array, device buffer or NULL) and on which stream the call runs;
what a row makes besides (a mapping handle, a likelihood handle) it reads back through the host-pointer calls of the
ABI and returns as `extras`.

`ROWS` together with `EXEMPT` is every `phmm_*` symbol that dbgphmm_amd/_ffi.py prototypes: test_caller_cases_cpu.py
holds that, so an entry point cannot be added without a row here or a written reason.

No torch: device memory and streams come from the HIP runtime the library is linked against, through ctypes."""
import contextlib
import ctypes as C
from collections import namedtuple

import numpy as np

HIP_SUCCESS, HIP_ERROR_NOT_READY = 0, 600
HIP_STREAM_NON_BLOCKING = 1
HIP_MEMCPY_D2H = 2
POISON = 0x55
SLACK = 64  # bytes behind every device output that must stay poisoned

# The work queued on a caller's stream in front of a call (test_callers_stream_same_bits): QUEUED_GIB memsets of one
# scratch buffer of 1 GiB.  See queue_work for the measurement behind the value.
SCRATCH_BYTES = 1 << 30
QUEUED_GIB = 4

_hip = None


def hip():
    """libamdhip64.so with the prototypes the two wrappers need (pointers and sizes are 64-bit: no default int)"""
    global _hip
    if _hip is None:
        h = C.CDLL("libamdhip64.so")
        vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int
        for name, args in {"hipMalloc": [C.POINTER(vp), sz], "hipFree": [vp], "hipMemset": [vp, i32, sz],
                           "hipMemcpy": [vp, vp, sz, i32], "hipMemsetAsync": [vp, i32, sz, vp],
                           "hipMemcpyAsync": [vp, vp, sz, i32, vp], "hipStreamCreateWithFlags": [C.POINTER(vp), C.c_uint],
                           "hipStreamQuery": [vp], "hipStreamSynchronize": [vp], "hipStreamDestroy": [vp]}.items():
            fn = getattr(h, name)
            fn.restype, fn.argtypes = i32, args
        _hip = h
    return _hip


class DeviceArray:
    """nbytes of device memory and `slack` bytes behind them, all filled with `fill` -- by a blocking hipMemset, or on
    `stream` behind whatever that stream already holds"""

    def __init__(self, nbytes, fill=POISON, slack=0, stream=None):
        self.nbytes, self.slack, self.fill = int(nbytes), int(slack), fill
        self.p = C.c_void_p()
        assert hip().hipMalloc(C.byref(self.p), max(self.nbytes + self.slack, 1)) == HIP_SUCCESS
        self.refill(stream)

    def refill(self, stream=None):
        n = max(self.nbytes + self.slack, 1)
        if stream is None:
            assert hip().hipMemset(self.p, self.fill, n) == HIP_SUCCESS
        else:
            stream.memset(self.p, self.fill, n)

    def bytes(self, stream=None):
        """every byte, slack included -> uint8; on `stream` the copy is queued there and the stream synchronised"""
        out = np.empty(self.nbytes + self.slack, dtype=np.uint8)
        if out.size:
            if stream is None:
                assert hip().hipMemcpy(out.ctypes.data_as(C.c_void_p), self.p, out.size, HIP_MEMCPY_D2H) == HIP_SUCCESS
            else:
                stream.copy_to_host(out, self.p)
                stream.synchronize()
        return out

    def numpy(self, dtype, stream=None):
        return self.bytes(stream)[:self.nbytes].view(dtype)

    def free(self):
        if self.p:
            hip().hipFree(self.p)
            self.p = C.c_void_p()

    def __del__(self):
        self.free()


class Stream:
    """a hipStreamNonBlocking stream: nothing on it is ordered against the NULL stream"""

    def __init__(self):
        self.s = C.c_void_p()
        assert hip().hipStreamCreateWithFlags(C.byref(self.s), HIP_STREAM_NON_BLOCKING) == HIP_SUCCESS
        assert self.s.value  # (a NULL handle would be the default stream)

    def memset(self, ptr, value, nbytes):
        assert hip().hipMemsetAsync(ptr, value, nbytes, self.s) == HIP_SUCCESS

    def copy_to_host(self, host_array, ptr):
        assert hip().hipMemcpyAsync(host_array.ctypes.data_as(C.c_void_p), ptr, host_array.nbytes, HIP_MEMCPY_D2H,
                                    self.s) == HIP_SUCCESS

    def query(self):
        return hip().hipStreamQuery(self.s)

    def synchronize(self):
        assert hip().hipStreamSynchronize(self.s) == HIP_SUCCESS

    def destroy(self):
        if self.s:
            hip().hipStreamDestroy(self.s)
            self.s = C.c_void_p()

    def __del__(self):
        self.destroy()


def queue_work(stream, scratch, gib=QUEUED_GIB):
    """`gib` memsets of the 1 GiB scratch buffer on `stream`: work that is still running when the library call behind
    it starts.  Measured on an idle MI355X, doubling from 1 GiB: hipStreamQuery right behind the memsets answered
    hipErrorNotReady at 1 GiB already, in every trial, so the doubling never came near its 16 GiB end.  The stream
    drains 1 GiB in 0.17 ms, 2 GiB in 0.33 ms, 4 GiB in 0.65 ms and 8 GiB in 1.3 ms (about 6 TB/s; MEASURED_DRAIN_MS);
    the host queues a memset in about 0.01 ms.  1 GiB would leave the host 0.1 ms for the poison fills of up to six
    outputs and the query that the stream case puts between the memsets and the call; the helper queues 4 GiB so that a
    loaded host still finds the stream busy."""
    assert scratch.nbytes == SCRATCH_BYTES
    for k in range(gib):
        stream.memset(scratch.p, k & 0xff, SCRATCH_BYTES)


MEASURED_DRAIN_MS = {1: 0.17, 2: 0.33, 4: 0.65, 8: 1.30}  # GiB queued -> ms until the stream is idle again


@contextlib.contextmanager
def on_stream(lib, stream):
    """phmm_set_stream(stream) for the body.  The setting is thread-local and outlives a test, so it goes back to the
    NULL stream whatever the body does, and the stream is drained before anything else may use its buffers."""
    handle = stream.s if isinstance(stream, Stream) else stream
    rc = lib.phmm_set_stream(handle)
    assert rc == 0, rc
    try:
        yield stream
    finally:
        lib.phmm_set_stream(None)
        if hasattr(stream, "synchronize"):
            stream.synchronize()


# ------------------------------------------------------------------------------------------------ the fixture
# an output of a row; host_only: the header names a host pointer; required: the header does not allow NULL
Out = namedtuple("Out", "name dtype shape host_only required", defaults=(False, False))
Row = namedtuple("Row", "name symbols outs call")


class Ctx:
    """The shared inputs: small_dbg_model(400, 12, 0.01, seed=21, min_copy_num=1) (458 nodes), 40 ragged reads of at
    most 80 bases (the recipe of test_run_dense_matches_oracle), their mapping lists from one
    generate_mappings(rc, None, True).  N = 458 is above warmup_threshold = 200, so the reads leave the dense warm-up
    after a few columns and walk the sparse kernels: `sparse_reads` counts those whose dense_columns < length
    (phmm_reads_last_call_info), and the GPU tests require at least one -- only then is the forward record pool used."""

    def __init__(self, genome=400, n_reads=40, seed_reads=40):
        import dbgphmm_amd as D
        from dbgphmm_amd import _ffi
        from helpers import small_dbg_model
        self.D, self.ffi, self.lib = D, _ffi, _ffi.lib()
        self.arrays, self.sg = small_dbg_model(genome, 12, 0.01, seed=21, min_copy_num=1)
        reads = D.sample_reads(self.arrays, 10 ** 9, 80, seed=seed_reads, max_reads=n_reads)
        self.reads = [r[: max(1, len(r) - (j * 7) % 31)] for j, r in enumerate(reads)]
        self.gm, self.rc = D.PHMMModel(self.arrays), D.ReadCollection(self.reads)
        self.mp, _ = self.gm.generate_mappings(self.rc, None, True)
        cols, _ = self.rc.last_call_info()
        self.sparse_reads = int((cols < np.array([len(r) for r in self.reads])).sum())
        self.R, self.N, self.E = len(self.reads), self.arrays.n_nodes, len(self.arrays.edge_src)
        self.bases = self.rc.total_bases()
        self.entries = int(self.lib.phmm_mappings_total_entries(self.mp._h))
        self.stride = int(self.arrays.param.n_max_gaps) + 2
        # candidates: two probability vectors, three copy-number vectors, three change lists (one of them empty)
        a = self.arrays
        self.cand_init = np.ascontiguousarray(np.stack([a.init_logp, a.init_logp]))
        self.cand_trans = np.ascontiguousarray(np.stack([a.trans_logp, a.trans_logp + np.log(0.5)]))
        self.cn = np.ascontiguousarray(self.sg.copy_num, dtype=np.uint32)
        nodes = np.unique(self.mp.arrays()[1])  # nodes some read maps to: their changes touch reads
        v0, v1, v2 = int(nodes[len(nodes) // 4]), int(nodes[len(nodes) // 2]), int(nodes[3 * len(nodes) // 4])
        self.chg_off = np.array([0, 1, 3, 3], dtype=np.uint64)
        self.chg_node = np.array([v0, v1, v2], dtype=np.uint32)
        self.chg_cn = (self.cn[self.chg_node] + 1).astype(np.uint32)
        self.cn_cands = np.ascontiguousarray(np.stack([self.cn] * 3))
        self.cn_cands[0, v0] += 1
        self.cn_cands[1, [v1, v2]] += 1
        self.move_node, self.move_cn = np.array([v0], dtype=np.uint32), np.array([self.cn[v0] + 1], dtype=np.uint32)
        self.id_off = np.arange(self.N + 1, dtype=np.uint32)
        self.id_nodes = np.arange(self.N, dtype=np.uint32)
        self.walks, self.walk_len = 50, 30


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _export(ctx, h):
    """what a mapping handle holds, through the host-pointer calls -> extras of the row"""
    L = ctx.lib
    tp, te = L.phmm_mappings_total_positions(h), L.phmm_mappings_total_entries(h)
    po, nd, lp = np.empty(tp + 1, dtype=np.uint64), np.empty(max(te, 1), dtype=np.uint32), np.empty(max(te, 1))
    ctx.ffi.check(L.phmm_mappings_export(h, _p(po), _p(nd), _p(lp)))
    lf, lb = np.empty(ctx.R), np.empty(ctx.R)
    ctx.ffi.check(L.phmm_mappings_read_logp(h, _p(lf), None))
    ctx.ffi.check(L.phmm_mappings_read_logp_backward(h, _p(lb), None))
    return {"mappings": (po, nd[:te], lp[:te]), "read_logp": lf, "read_logp_backward": lb}


def _generate(ctx, b, carried, keep=None):
    h = C.c_void_p()
    ctx.ffi.check(ctx.lib.phmm_generate_mappings(ctx.gm._h, ctx.rc._h, ctx.mp._h if carried else None, 1, C.byref(h),
                                                 b["node_freq"]))
    try:
        return _export(ctx, h)
    finally:
        if keep is not None:
            keep.append(h)  # the caller destroys it (the spare-buffer variant decides when)
        else:
            ctx.lib.phmm_mappings_destroy(h)


def _map_nodes(ctx, b):
    h = C.c_void_p()
    ctx.ffi.check(ctx.lib.phmm_mappings_map_nodes(ctx.gm._h, ctx.rc._h, ctx.mp._h, _p(ctx.id_off), _p(ctx.id_nodes),
                                                  ctx.N, C.byref(h)))
    try:
        return _export(ctx, h)
    finally:
        ctx.lib.phmm_mappings_destroy(h)


@contextlib.contextmanager
def _likelihood(ctx):
    h = C.c_void_p()
    ctx.ffi.check(ctx.lib.phmm_likelihood_create(ctx.gm._h, ctx.rc._h, ctx.mp._h, _p(ctx.cn), 1, C.byref(h)))
    try:
        yield h
    finally:
        ctx.lib.phmm_likelihood_destroy(h)


def _lk_create(ctx, b):
    with _likelihood(ctx) as h:  # what the handle holds after the create alone
        ctx.ffi.check(ctx.lib.phmm_likelihood_current(h, b["copy_nums"], b["logp"], b["total"]))


def _lk_score(ctx, b):
    with _likelihood(ctx) as h:  # (after a move: the candidates are scored against what the move left)
        ctx.ffi.check(ctx.lib.phmm_likelihood_move(h, 1, _p(ctx.move_node), _p(ctx.move_cn), None, None))
        ctx.ffi.check(ctx.lib.phmm_likelihood_score_changes(h, 3, _p(ctx.chg_off), _p(ctx.chg_node), _p(ctx.chg_cn),
                                                            b["logp"], b["total"], b["n_rescored"]))


def _lk_move(ctx, b):
    with _likelihood(ctx) as h:
        ctx.ffi.check(ctx.lib.phmm_likelihood_move(h, 1, _p(ctx.move_node), _p(ctx.move_cn), b["total"], b["n_rescored"]))


def _lk_current(ctx, b):
    with _likelihood(ctx) as h:
        ctx.ffi.check(ctx.lib.phmm_likelihood_move(h, 1, _p(ctx.move_node), _p(ctx.move_cn), None, None))
        ctx.ffi.check(ctx.lib.phmm_likelihood_current(h, b["copy_nums"], b["logp"], b["total"]))


def _ck(f):
    """row body: one ABI call whose status is checked"""
    def call(ctx, b):
        ctx.ffi.check(f(ctx, ctx.lib, b))
    return call


def _full_prob(hinted, ratio):
    return _ck(lambda c, L, b: L.phmm_full_prob_reads(c.gm._h, c.rc._h, c.mp._h if hinted else None, ratio, b["logp"], b["total"]))


F8, U4, U8, U1 = np.float64, np.uint32, np.uint64, np.uint8
_LOGP_TOTAL = lambda c: [Out("logp", F8, (c.R,)), Out("total", F8, (1,))]
_LK_STATE = lambda c: [Out("copy_nums", U4, (c.N,), True), Out("logp", F8, (c.R,)), Out("total", F8, (1,))]

ROWS = [
    Row("run_dense", ["phmm_run_dense"],
        lambda c: [Out("logp_forward", F8, (c.R,), False, True), Out("logp_backward", F8, (c.R,)), Out("node_freq", F8, (c.N,))],
        _ck(lambda c, L, b: L.phmm_run_dense(c.gm._h, c.rc._h, b["logp_forward"], b["logp_backward"], b["node_freq"]))),
    Row("run_dense_edges", ["phmm_run_dense_edges"],
        lambda c: [Out("logp_forward", F8, (c.R,)), Out("edge_freq", F8, (c.E,)), Out("init_freq", F8, (c.N,))],
        _ck(lambda c, L, b: L.phmm_run_dense_edges(c.gm._h, c.rc._h, b["logp_forward"], b["edge_freq"], b["init_freq"]))),
    Row("run_sparse", ["phmm_run_sparse"],
        lambda c: [Out("logp_forward", F8, (c.R,)), Out("logp_backward", F8, (c.R,)), Out("node_freq", F8, (c.N,))],
        _ck(lambda c, L, b: L.phmm_run_sparse(c.gm._h, c.rc._h, b["logp_forward"], b["logp_backward"], b["node_freq"]))),
    Row("full_prob_sparse_backward", ["phmm_full_prob_sparse_backward"], _LOGP_TOTAL,
        _ck(lambda c, L, b: L.phmm_full_prob_sparse_backward(c.gm._h, c.rc._h, b["logp"], b["total"]))),
    Row("full_prob_reads", ["phmm_full_prob_reads"], _LOGP_TOTAL, _full_prob(False, 1)),
    Row("full_prob_reads_topk", ["phmm_full_prob_reads"], _LOGP_TOTAL, _full_prob(False, 0)),
    Row("full_prob_reads_hinted", ["phmm_full_prob_reads"], _LOGP_TOTAL, _full_prob(True, 1)),
    Row("full_prob_reads_candidates", ["phmm_full_prob_reads_candidates"],
        lambda c: [Out("logp", F8, (2, c.R)), Out("total", F8, (2,), False, True)],
        _ck(lambda c, L, b: L.phmm_full_prob_reads_candidates(c.gm._h, c.rc._h, c.mp._h, 2, _p(c.cand_init), _p(c.cand_trans),
                                                              b["logp"], b["total"]))),
    Row("full_prob_reads_copy_nums", ["phmm_full_prob_reads_copy_nums"],
        lambda c: [Out("logp", F8, (3, c.R)), Out("total", F8, (3,), False, True)],
        _ck(lambda c, L, b: L.phmm_full_prob_reads_copy_nums(c.gm._h, c.rc._h, c.mp._h, 3, _p(c.cn_cands), 1, b["logp"],
                                                             b["total"]))),
    Row("full_prob_reads_copy_num_changes", ["phmm_full_prob_reads_copy_num_changes"],
        lambda c: [Out("logp", F8, (3, c.R)), Out("total", F8, (3,)), Out("n_rescored", U8, (3,))],
        _ck(lambda c, L, b: L.phmm_full_prob_reads_copy_num_changes(c.gm._h, c.rc._h, c.mp._h, _p(c.cn), 1, 3, _p(c.chg_off),
                                                                    _p(c.chg_node), _p(c.chg_cn), b["logp"], b["total"],
                                                                    b["n_rescored"]))),
    Row("generate_mappings", ["phmm_generate_mappings"], lambda c: [Out("node_freq", F8, (c.N,))],
        lambda c, b: _generate(c, b, False)),
    Row("generate_mappings_carried", ["phmm_generate_mappings"], lambda c: [Out("node_freq", F8, (c.N,))],
        lambda c, b: _generate(c, b, True)),
    Row("mappings_read_logp", ["phmm_mappings_read_logp"], _LOGP_TOTAL,
        _ck(lambda c, L, b: L.phmm_mappings_read_logp(c.mp._h, b["logp"], b["total"]))),
    Row("mappings_read_logp_backward", ["phmm_mappings_read_logp_backward"], _LOGP_TOTAL,
        _ck(lambda c, L, b: L.phmm_mappings_read_logp_backward(c.mp._h, b["logp"], b["total"]))),
    Row("mappings_node_freqs", ["phmm_mappings_node_freqs"], lambda c: [Out("freq", F8, (c.N,), False, True)],
        _ck(lambda c, L, b: L.phmm_mappings_node_freqs(c.mp._h, c.N, b["freq"]))),
    Row("mappings_map_nodes", ["phmm_mappings_map_nodes"], lambda c: [], _map_nodes),
    Row("run_with_mapping_edges", ["phmm_run_with_mapping_edges"],
        lambda c: [Out("logp_forward", F8, (c.R,)), Out("edge_freq", F8, (c.E,)), Out("init_freq", F8, (c.N,))],
        _ck(lambda c, L, b: L.phmm_run_with_mapping_edges(c.gm._h, c.rc._h, c.mp._h, b["logp_forward"], b["edge_freq"],
                                                          b["init_freq"]))),
    Row("run_with_mapping_states", ["phmm_run_with_mapping_states"],
        lambda c: [Out("logp_forward", F8, (c.R,)), Out("state_logp", F8, (c.entries, 3)), Out("best", U4, (c.bases,))],
        _ck(lambda c, L, b: L.phmm_run_with_mapping_states(c.gm._h, c.rc._h, c.mp._h, b["logp_forward"], b["state_logp"],
                                                           b["best"]))),
    Row("run_with_mapping_best_path", ["phmm_run_with_mapping_best_path"],
        lambda c: [Out("logp", F8, (c.R,)), Out("path", U4, (c.bases, c.stride)), Out("counts", U4, (c.R, 4))],
        _ck(lambda c, L, b: L.phmm_run_with_mapping_best_path(c.gm._h, c.rc._h, c.mp._h, b["logp"], b["path"], b["counts"]))),
    Row("run_with_mapping_sample_paths", ["phmm_run_with_mapping_sample_paths"],
        lambda c: [Out("logp", F8, (c.R,)), Out("path_logp", F8, (c.R, 3)), Out("path", U4, (3, c.bases, c.stride)),
                   Out("counts", U4, (c.R, 3, 4)), Out("node_usage", U4, (3, c.N))],
        _ck(lambda c, L, b: L.phmm_run_with_mapping_sample_paths(c.gm._h, c.rc._h, c.mp._h, 3, 77, b["logp"], b["path_logp"],
                                                                 b["path"], b["counts"], b["node_usage"]))),
    Row("sample_reads", ["phmm_sample_reads"],
        lambda c: [Out("bases", U1, (c.walks, c.walk_len + 1)), Out("len", U4, (c.walks,)), Out("flags", U4, (c.walks,)),
                   Out("history", U4, (c.walks, c.walk_len + 1)), Out("history_len", U4, (c.walks,)),
                   Out("node_usage", U4, (c.N,))],
        _ck(lambda c, L, b: L.phmm_sample_reads(c.gm._h, 0, c.walks, c.walk_len, 0, None, 0, 3, b["bases"], b["len"], b["flags"],
                                                b["history"], c.walk_len + 1 if b["history"] is not None else 0,
                                                b["history_len"], b["node_usage"]))),
    Row("likelihood_create", ["phmm_likelihood_create"], _LK_STATE, _lk_create),
    Row("likelihood_score_changes", ["phmm_likelihood_score_changes"],
        lambda c: [Out("logp", F8, (3, c.R)), Out("total", F8, (3,)), Out("n_rescored", U8, (3,))], _lk_score),
    Row("likelihood_move", ["phmm_likelihood_move"], lambda c: [Out("total", F8, (1,)), Out("n_rescored", U8, (1,))], _lk_move),
    Row("likelihood_current", ["phmm_likelihood_current"], _LK_STATE, _lk_current),
]
ROW = {r.name: r for r in ROWS}

# Every other prototyped symbol, with the reason it has no row: it computes nothing on the device into a caller's
# output, so there is no stream or output form to vary.
EXEMPT = {
    "phmm_last_error": "phmm_last_*: reads the thread's last message, no device work",
    "phmm_last_call_stats": "phmm_last_*: reads the thread's counters of the last call, no device work",
    "phmm_last_call_prefix_share": "phmm_last_*: reads the thread's counters of the last call, no device work",
    "phmm_version": "returns a constant string",
    "phmm_device_count": "handle / device count: no stream, no output array",
    "phmm_reads_count": "handle count: a field of the handle",
    "phmm_reads_total_bases": "handle count: a field of the handle",
    "phmm_model_n_nodes": "handle count: a field of the handle",
    "phmm_model_n_edges": "handle count: a field of the handle",
    "phmm_mappings_total_positions": "handle count: a field of the handle",
    "phmm_mappings_total_entries": "handle count: a field of the handle",
    "phmm_set_device": "setter: selects the device of the thread",
    "phmm_set_stream": "setter: the knob under test, exercised by every stream case",
    "phmm_set_workspace_limit": "setter: exercised by the chunked variants of the repeated-call case",
    "phmm_enable_timing": "setter: instrumentation switch",
    "phmm_release_workspace": "workspace control, synchronises the device by contract; no output",
    "phmm_workspace_bytes": "workspace control: the quantity the repeated-call case asserts on",
    "phmm_params_new": "host arithmetic into a host struct",
    "phmm_params_uniform": "host arithmetic into a host struct",
    "phmm_model_create": "handle create: blocking uploads of host inputs, no output array",
    "phmm_model_set_probs": "setter on a handle: uploads host inputs, no output array",
    "phmm_model_set_params": "setter on a handle: uploads host inputs, no output array",
    "phmm_model_destroy": "handle destroy: frees what the handle owns, no output",
    "phmm_reads_create": "handle create: host copy of host inputs",
    "phmm_reads_destroy": "handle destroy: frees what the handle owns, no output",
    "phmm_reads_last_call_info": "host arrays kept by the handle, host pointers by the header; the fixture reads it",
    "phmm_mappings_create": "handle create: host copy of host inputs",
    "phmm_mappings_export": "host pointers by the header; every row that makes mappings is read back through it",
    "phmm_mappings_destroy": "handle destroy; the spare-buffer variant of the repeated-call case covers its pool path",
    "phmm_likelihood_destroy": "handle destroy: frees what the handle owns, no output",
    "phmm_likelihood_refresh": "no output: the full rescoring phmm_likelihood_create runs, which has a row",
    "phmm_likelihood_set_groups": "setter on a handle: uploads host inputs, no output array",
    "phmm_likelihood_score_group_changes": "the group flavour of phmm_likelihood_score_changes: same output writers, "
                                           "held bit-equal to the node form by test_gpu_likelihood_groups.py",
    "phmm_likelihood_move_groups": "the group flavour of phmm_likelihood_move: same output writers, held bit-equal to "
                                   "the node form by test_gpu_likelihood_groups.py",
    "phmm_likelihood_current_groups": "host copy of a host array of the handle, host pointer by the header",
    "phmm_dense_tables": "single-read table dump for parity tools, host pointers by the header",
    "phmm_backward_sparse_tables": "single-read table dump for parity tools, host pointers by the header",
    "phmm_q_score_exact": "O(N + E) on the host from host inputs, host pointers by the header",
}


def prototyped_symbols():
    """the phmm_* names dbgphmm_amd/_ffi.py binds: its closed table and the companion headers' additions"""
    from dbgphmm_amd import _ffi
    return set(_ffi.DECLARED_SYMBOLS) | {s for syms in _ffi.EXTENSION_SYMBOLS.values() for s in syms}


# ------------------------------------------------------------------------------------------------ running a row
def optional_outputs(ctx, row):
    return [o.name for o in row.outs(ctx) if not o.required]


def run_host(ctx, row, null=()):
    """the row with host outputs (NULL for the names in `null`) -> {name: array} with the row's extras merged in"""
    outs = row.outs(ctx)
    arrays = {o.name: np.zeros(o.shape, dtype=o.dtype) for o in outs}
    extras = row.call(ctx, {o.name: None if o.name in null else _p(arrays[o.name]) for o in outs}) or {}
    return {**{k: v for k, v in arrays.items() if k not in null}, **extras}


class DeviceOutputs:
    """device buffers for the row's outputs (host arrays for the host-only ones), poisoned, with slack behind each"""

    def __init__(self, ctx, row, stream=None):
        self.outs, self.stream = row.outs(ctx), stream
        self.dev = {o.name: DeviceArray(int(np.prod(o.shape)) * np.dtype(o.dtype).itemsize, POISON, SLACK, stream)
                    for o in self.outs if not o.host_only}
        self.host = {o.name: np.zeros(o.shape, dtype=o.dtype) for o in self.outs if o.host_only}

    def poison(self, stream):
        """the poison fills again, queued on `stream` behind what it holds"""
        for d in self.dev.values():
            d.refill(stream)

    def pointers(self):
        return {o.name: _p(self.host[o.name]) if o.host_only else self.dev[o.name].p for o in self.outs}

    def read(self):
        """-> ({name: array}, True when the slack behind every output still holds the poison)"""
        got, clean = dict(self.host), True
        for o in self.outs:
            if o.host_only:
                continue
            raw = self.dev[o.name].bytes(self.stream)
            n = self.dev[o.name].nbytes
            got[o.name] = raw[:n].view(o.dtype).reshape(o.shape)
            clean = clean and bool(np.all(raw[n:] == POISON))
        return got, clean

    def free(self):
        for d in self.dev.values():
            d.free()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_result(want, got, tolerance=None):
    """Every output of `got` against the reference form's: the raw bits (so -inf equals -inf and a NaN its own bit
    pattern).  The mapping lists of a row compare under helpers.same_mappings, as in the tests that pin
    generate_mappings itself: offsets and values bit-equal, two near-equal entries of one list may trade places.
    `tolerance` {name: atol} is for outputs that are not bit-reproducible from call to call (see the GPU test).
    -> list of the names that differ"""
    from helpers import same_mappings
    bad = []
    for k, w in want.items():
        if k not in got:
            continue
        g = got[k]
        if k == "mappings":
            ok = same_mappings(w, g)
        elif tolerance and k in tolerance:
            with np.errstate(invalid="ignore"):
                ok = w.shape == g.shape and bool(np.all((w == g) | (np.abs(w - g) <= tolerance[k])))
        else:
            ok = same_bits(np.asarray(w), np.asarray(g))
        if not ok:
            bad.append(k)
    return bad
