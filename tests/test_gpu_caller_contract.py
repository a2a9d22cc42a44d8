"""GPU: the calling forms a host program uses -- its own stream, device output buffers, the same call many times --
held to the form every other GPU test uses: once, on the NULL stream, into host arrays.

The reference of a row (tests/caller_cases.py) is that row run once on the NULL stream with host outputs; the files
that pin the entry points to the oracle are the other test_gpu_*.py.  Outputs are compared on their raw bits; the
mapping lists a row makes compare under helpers.same_mappings, as in the tests of generate_mappings itself (two
near-equal entries of one list may trade places).

Bit-reproducibility: every row was run twice on the NULL stream on an MI355X before the cases below were written.
Every output of every row came back with the same bits but one: node_freq of run_sparse, which its kernels sum over
the reads with floating-point atomics in whatever order the waves arrive.  It takes the tolerance of its own parity
test (test_gpu_sparse.py::test_run_sparse_node_freqs_match_oracle, the TOL_FREQ of tests/test_gpu_dense.py): 1e-9 x
n_reads.  A row found not to be reproducible later is entered in TOLERANT with its existing test's tolerance --
1e-9 on ln P, 1e-9 x n_reads on frequencies -- and the reason; no other tolerance is used here.

  a. device outputs, poisoned with 0x55 and 64 bytes of slack behind each, equal the host outputs; the slack stays;
     the row also runs with every optional output NULL;
  b. the same on a fresh hipStreamNonBlocking stream that is still busy with queued memsets when the call is made,
     read back on that stream alone (no device-wide synchronisation anywhere in the case);
  c. calls alternate between two such streams with nothing in between: the workspaces belong to the device;
  d. the stream setting is per thread;
  e. the worker pipeline (worker threads with streams of their own) under a caller's stream;
  f. four calls in a row: phmm_workspace_bytes() is the same after calls 2, 3 and 4, exactly, and so are the outputs.
     Before the forward record pool's 4 KB over-fetch pad was kept out of its capacity feedback (sparse_dyn.hip), the
     un-hinted generate_mappings and full_prob_reads rows grew by 4096 bytes per chunk and call here."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import caller_cases as cc
from dbgphmm_amd import _ffi

pytestmark = pytest.mark.gpu
NAMES = [row.name for row in cc.ROWS]
# row name -> {output: atol as a function of n_reads}: outputs that are not bit-reproducible from call to call
TOLERANT = {"run_sparse": {"node_freq": lambda n_reads: 1e-9 * n_reads}}  # atomic adds over the reads, in arrival order
WORKERS_ENV = {"PHMM_WORKERS": "2", "PHMM_PIPELINE_MIN_GROUPS": "1", "PHMM_CHUNK_GROUPS": "2"}  # test_gpu_prefix_share.py
JOIN_S = 120


class _Refs:
    """the reference form of every row of one fixture, computed once and never written to"""

    def __init__(self, ctx):
        self.ctx, self.cache = ctx, {}

    def __call__(self, name):
        if name not in self.cache:
            self.cache[name] = cc.run_host(self.ctx, cc.ROW[name])
            for v in self.cache[name].values():
                for a in (v if isinstance(v, tuple) else (v,)):
                    a.setflags(write=False)
        return self.cache[name]


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    c = cc.Ctx()
    assert c.sparse_reads >= 1, "no read left the dense warm-up: the forward record pool would not be used"
    return c


@pytest.fixture(scope="module")
def refs(ctx):
    return _Refs(ctx)


@pytest.fixture(scope="module")
def many(gpu_lib):
    """100 reads on the same model: 13 read groups of 8, seven chunks under PHMM_CHUNK_GROUPS=2"""
    c = cc.Ctx(n_reads=100, seed_reads=41)
    assert c.R == 100 and c.sparse_reads >= 1
    return c


@pytest.fixture(scope="module")
def wide(gpu_lib):
    """192 reads on small_dbg_model(2000, 12, 0.01, seed=21, min_copy_num=1): three read groups of 64 whose dense
    tables (at least 12 columns x 24 bytes + 32 bytes per node and lane) take more than half of the 64 MB a call plans
    with at the least, so that a workspace limit of 64 MB gives every group a chunk of its own"""
    c = cc.Ctx(genome=2000, n_reads=192, seed_reads=42)
    assert c.R == 192 and c.sparse_reads >= 1
    assert (12 * 24 + 32) * c.N * 64 > (64 << 20) // 2
    return c


@pytest.fixture(scope="module")
def scratch(gpu_lib):
    d = cc.DeviceArray(cc.SCRATCH_BYTES, 0)
    yield d
    d.free()


def _differs(name, want, got, n_reads=40):
    tol = {k: f(n_reads) for k, f in TOLERANT.get(name, {}).items()}
    return cc.same_result(want, got, tol)


def _run_on_device_outputs(c, row, stream=None, scratch=None):
    """the row into poisoned device buffers; with a stream: inside on_stream, behind queued work
    -> (outputs and extras, slack clean, what hipStreamQuery said right before the call)"""
    d = cc.DeviceOutputs(c, row)  # (allocated and filled before anything is queued: hipMalloc is not stream-ordered)
    try:
        if stream is None:
            extras = row.call(c, d.pointers()) or {}
            got, clean = d.read()
            return {**got, **extras}, clean, None
        d.stream = stream
        with cc.on_stream(c.lib, stream):
            cc.queue_work(stream, scratch)
            d.poison(stream)
            busy = stream.query()
            extras = row.call(c, d.pointers()) or {}
            got, clean = d.read()  # hipMemcpyAsync on the stream, then hipStreamSynchronize(stream)
        return {**got, **extras}, clean, busy
    finally:
        d.free()


# ------------------------------------------------------------------ a. device outputs
@pytest.mark.parametrize("name", NAMES)
def test_device_outputs_equal_host_outputs(ctx, refs, name):
    row, want = cc.ROW[name], refs(name)
    got, clean, _ = _run_on_device_outputs(ctx, row)
    assert not _differs(name, want, got), _differs(name, want, got)
    assert clean, "bytes behind an output's extent were written"
    optional = cc.optional_outputs(ctx, row)
    if optional:
        rest = cc.run_host(ctx, row, null=optional)
        assert not _differs(name, want, rest), _differs(name, want, rest)


# ------------------------------------------------------------------ b. a caller's stream that is still busy
@pytest.mark.parametrize("name", NAMES)
def test_callers_stream_same_bits(ctx, refs, scratch, name):
    row, want = cc.ROW[name], refs(name)
    s = cc.Stream()
    try:
        got, clean, busy = _run_on_device_outputs(ctx, row, s, scratch)
    finally:
        s.destroy()
    assert busy == cc.HIP_ERROR_NOT_READY, "the queued work had drained before the call: the case ordered nothing"
    assert not _differs(name, want, got), _differs(name, want, got)
    assert clean


# ------------------------------------------------------------------ c. two streams, one device workspace
def test_two_streams_share_the_workspace(ctx, refs):
    names = ["run_dense", "generate_mappings", "full_prob_reads_hinted", "run_with_mapping_best_path",
             "likelihood_score_changes"] * 2
    streams = [cc.Stream(), cc.Stream()]
    outs = [cc.DeviceOutputs(ctx, cc.ROW[n]) for n in names]
    extras = []
    try:
        try:
            for k, (n, d) in enumerate(zip(names, outs)):
                s = streams[k % 2]  # never the stream of the call before
                assert ctx.lib.phmm_set_stream(s.s) == 0
                d.stream = s
                d.poison(s)
                extras.append(cc.ROW[n].call(ctx, d.pointers()) or {})
        finally:
            ctx.lib.phmm_set_stream(None)
        for k, (n, d) in enumerate(zip(names, outs)):
            got, clean = d.read()  # on the call's own stream
            assert not _differs(n, refs(n), {**got, **extras[k]}), (k, n, _differs(n, refs(n), {**got, **extras[k]}))
            assert clean, (k, n)
    finally:
        for s in streams:
            s.synchronize()
        for d in outs:
            d.free()
        for s in streams:
            s.destroy()


# ------------------------------------------------------------------ d. the setting is per thread
def _in_thread(f):
    box = {}

    def body():
        try:
            box["value"] = f()
        except BaseException as e:  # (reported by the joining thread)
            box["error"] = e
    t = threading.Thread(target=body, daemon=True)
    t.start()
    return t, box


def _joined(t, box):
    t.join(JOIN_S)
    assert not t.is_alive(), "the thread did not come back"
    if "error" in box:
        raise box["error"]
    return box["value"]


def test_stream_is_per_thread(ctx, refs, scratch):
    hinted, dense = cc.ROW["full_prob_reads_hinted"], cc.ROW["run_dense"]
    want_h, want_d = refs("full_prob_reads_hinted"), refs("run_dense")
    main = cc.Stream()
    try:
        with cc.on_stream(ctx.lib, main):
            # a thread that never set a stream: the NULL stream, whatever this thread holds
            got = _joined(*_in_thread(lambda: cc.run_host(ctx, hinted)))
            assert not _differs(hinted.name, want_h, got)
            # ... and this thread's setting is still `main`: were it NULL, the call below would write its outputs at
            # once and the poison fills queued behind the memsets would land on top of them
            d = cc.DeviceOutputs(ctx, hinted)
            try:
                d.stream = main
                cc.queue_work(main, scratch)
                d.poison(main)
                busy = main.query()
                hinted.call(ctx, d.pointers())
                got, clean = d.read()
            finally:
                main.synchronize()
                d.free()
            assert busy == cc.HIP_ERROR_NOT_READY
            assert not _differs(hinted.name, want_h, got) and clean

            # two threads, a stream each, at the same time: the library serialises the calls
            def other():
                s = cc.Stream()
                try:
                    return _run_on_device_outputs(ctx, dense, s, other_scratch)
                finally:
                    s.destroy()
            other_scratch = scratch  # (memsets of one scratch buffer from two streams: its contents are never read)
            t, box = _in_thread(other)
            mine = [cc.run_host(ctx, hinted) for _ in range(3)]
            got_d, clean_d, _ = _joined(t, box)
            assert not _differs(dense.name, want_d, got_d) and clean_d
            for got in mine:
                assert not _differs(hinted.name, want_h, got)
    finally:
        main.destroy()


# ------------------------------------------------------------------ e. worker threads under a caller's stream
def test_worker_pipeline_on_a_callers_stream(many, scratch):
    row = cc.ROW["generate_mappings"]
    saved = {k: os.environ.get(k) for k in WORKERS_ENV}
    os.environ.update(WORKERS_ENV)  # (the library reads its knobs at every call)
    s = cc.Stream()
    try:
        want = cc.run_host(many, row)
        got, clean, busy = _run_on_device_outputs(many, row, s, scratch)
    finally:
        s.destroy()
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    assert busy == cc.HIP_ERROR_NOT_READY
    assert not _differs(row.name, want, got), _differs(row.name, want, got)
    assert clean


# ------------------------------------------------------------------ f. the steady state
def _four_calls(c, name, call=None):
    """-> workspace bytes after calls 2, 3, 4; asserts the outputs of calls 2-4 equal call 1"""
    call = call or (lambda: cc.run_host(c, cc.ROW[name]))
    first, held = call(), []
    for k in (2, 3, 4):
        got = call()
        held.append(int(c.lib.phmm_workspace_bytes()))
        assert not _differs(name, first, got), (k, _differs(name, first, got))
    return held


@pytest.mark.parametrize("name", NAMES)
def test_repeated_calls_hold_the_workspace(ctx, name):
    held = _four_calls(ctx, name)
    print(name, "workspace bytes after calls 2-4:", held)
    assert held[0] == held[1] == held[2], [h - held[0] for h in held]


@pytest.mark.parametrize("name", ["generate_mappings", "full_prob_reads"])
def test_repeated_calls_in_chunks_hold_the_workspace(wide, name):
    """under a workspace limit that cuts the call into three chunks: every chunk reserves the record pool again"""
    L = wide.lib
    cc.run_host(wide, cc.ROW[name])
    one_chunk = _ffi.last_call_stats(_ffi.PHMM_STATS_DENSE_FWD)[1]
    _ffi.check(L.phmm_set_workspace_limit(64 << 20))
    try:
        held = _four_calls(wide, name)
        dense = _ffi.last_call_stats(_ffi.PHMM_STATS_DENSE_FWD)[1]
        sparse = _ffi.last_call_stats(_ffi.PHMM_STATS_SPARSE_FWD)[1]
    finally:
        _ffi.check(L.phmm_set_workspace_limit(0))
    print(name, "dense forward launches", one_chunk, "->", dense, "sparse forward launches", sparse, "bytes", held)
    # three chunks (the arithmetic of the `wide` fixture): a dense forward step at least and the sparse phases A and B
    # in each, and more dense forward steps than the one chunk of the unlimited call took
    assert dense >= 3 and dense > one_chunk and sparse >= 6, (one_chunk, dense, sparse)
    assert held[0] == held[1] == held[2], [h - held[0] for h in held]


@pytest.mark.parametrize("keep", [False, True], ids=["destroyed_before_the_next_call", "kept_alive"])
def test_repeated_generate_mappings_and_their_handles(wide, keep):
    """the spare-buffer path: the device arrays of a destroyed Mappings go to the pool and into the next call's result.
    The bytes are taken after each call and after each destroy; `kept_alive` destroys nothing until the end."""
    L, row = wide.lib, cc.ROW["generate_mappings"]
    handles, after_call, after_del, first = [], [], [], None
    out = np.zeros(wide.N)
    try:
        for k in range(4):
            got = cc._generate(wide, {"node_freq": out.ctypes.data_as(C.c_void_p)}, False, keep=handles)
            got["node_freq"] = out.copy()
            after_call.append(int(L.phmm_workspace_bytes()))
            if not keep:
                L.phmm_mappings_destroy(handles.pop())
                after_del.append(int(L.phmm_workspace_bytes()))
            first = first or got
            assert not _differs(row.name, first, got), (k, _differs(row.name, first, got))
    finally:
        for h in handles:
            L.phmm_mappings_destroy(h)
    print("after calls", after_call, "after destroys", after_del)
    assert after_call[1] == after_call[2] == after_call[3], after_call
    if not keep:
        assert after_del[1] == after_del[2] == after_del[3], after_del
