"""GPU: reads drawn from the model on the device (phmm_sample_reads, PHMMModel.sample_reads).

The call is held to tests/sample_reads_ref.py, the header's walk, random stream and draw rule in plain Python (held on
its own by tests/test_sample_reads_ref_cpu.py):
  * bases, lengths, flags, histories and history lengths equal the restatement's WORD FOR WORD on the shared fixtures.
    The device's exp and Python's may differ in the last bits, so this needs every decision to stay clear of its
    boundaries: the CPU test asserts a margin of 1e-9 of every fixture (a condition on the inputs);
  * 40 000 of the device's walks pass the chi-square against the exact law of the tiny model;
  * a walk's bits do not depend on first_index splits, on the outputs requested or where they live, on chunks, on a
    second call, or on other numbers set in between;
  * the truth of a walk is a path of the forward model: the best path over its lists scores no less, and the full
    probability over the same lists no less than that."""
import ctypes as C
import math

import numpy as np
import pytest

import dbgphmm_amd as D
import best_path_ref as B
import sample_reads_ref as G
from dbgphmm_amd import _ffi

pytestmark = pytest.mark.gpu
NINF = -math.inf
STATS = 2


def _cap(f):
    return (G.state_cap(f["length"]) if f["kind"] == G.EMIT_COUNT else f["length"]) + 2


def _raw(gm, first, n, length, kind, start=None, seed=0, history_cap=0, usage=False, fill=0x77):
    """one call through the C ABI with sentinel-filled host outputs -> (rc, bases, len, flags, history, history_len, usage)"""
    sn = None if start is None else np.ascontiguousarray(start, dtype=np.uint32)
    bases = np.full((n, length + 1), fill, dtype=np.uint8)
    ln, fl, hl = (np.full(n, 0x77777777, dtype=np.uint32) for _ in range(3))
    hist = np.full((n, history_cap), 0x77777777, dtype=np.uint32) if history_cap else None
    use = np.full(gm.n_nodes, 0x77777777, dtype=np.uint32) if usage else None
    P = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
    rc = _ffi.lib().phmm_sample_reads(gm._h, first, n, length, kind, P(sn), 0 if sn is None else sn.size, seed, P(bases), P(ln),
                                      P(fl), P(hist), history_cap, P(hl), P(use))
    return rc, bases, ln, fl, hist, hl, use


def _ok(*a, **kw):
    out = _raw(*a, **kw)
    _ffi.check(out[0])
    return out[1:]


def _same(x, y):
    return all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(x, y))


# ------------------------------------------------------------------ 1. word for word against the restatement
@pytest.fixture(scope="module")
def models(gpu_lib):
    return {name: D.PHMMModel(G.model(name)) for name in G.MODELS}


@pytest.mark.parametrize("k", range(len(G.fixtures())), ids=[f["tag"] for f in G.fixtures()])
def test_word_for_word(models, k):
    f = G.fixtures()[k]
    want = G.fixture_walks(k)
    gm = models[f["tag"].split()[0]]
    cap, n, L = _cap(f), f["n_walks"], f["length"]
    bases, ln, fl, hist, hl, use = _ok(gm, f["first_index"], n, L, f["kind"], f["start_nodes"], f["seed"], cap, True)
    for w, (b, h, flags, _) in enumerate(want):
        if hist[w, :len(h)].tolist() != h or hl[w] != len(h):
            raise AssertionError(f"{f['tag']}: " + G.first_difference(f["arrays"], f["seed"], f["first_index"] + w, L, f["kind"],
                                                                      f["start_nodes"], hist[w]))
        assert np.all(hist[w, len(h):] == G.NONE), (f["tag"], w)
        assert ln[w] == len(b) and bases[w, :len(b)].tobytes() == b and not bases[w, len(b):].any(), (f["tag"], w)
        assert fl[w] == flags, (f["tag"], w, fl[w], flags)
    assert np.array_equal(use, G.usage_of([h for _, h, _, _ in want], gm.n_nodes)), f["tag"]
    ms, launches, cells = _ffi.last_call_stats(STATS)
    assert launches == 1 and cells == sum(len(h) for _, h, _, _ in want) - (n if f["start_nodes"] else 0)


# ------------------------------------------------------------------ 2. the exact law
def test_chi_square_of_the_gpus_walks(gpu_lib):
    arrays, length, kind = G.chi_case()
    law = G.exact_law(arrays, length, kind)
    gm = D.PHMMModel(arrays)
    bases, ln, fl, hist, hl, _ = _ok(gm, 0, G.CHI_WALKS, length, kind, None, G.CHI_SEED, length + 1)
    outcomes = [(tuple(hist[w, :hl[w]].tolist()), bases[w, :ln[w]].tobytes()) for w in range(G.CHI_WALKS)]
    chi, df = G.chi_square(law, outcomes)
    print(f"{len(law)} outcomes, chi-square {chi:.1f} at df {df}, bar {G.chi_bar(df):.1f}")
    assert df >= 50 and chi <= G.chi_bar(df)


# ------------------------------------------------------------------ 3. the same bits whatever surrounds a walk
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


@pytest.fixture(scope="module")
def zoo_run(models):
    gm = models["zoo"]
    args = dict(length=63, kind=G.ENDABLE, start=None, seed=77, history_cap=66, usage=True)
    return gm, args, _ok(gm, 0, 130, **args)


def test_first_index_splits(zoo_run):
    gm, args, whole = zoo_run
    for step in (1, 7, 64):
        parts = [_ok(gm, w0, min(step, 130 - w0), **{**args, "usage": False}) for w0 in range(0, 130, step)]
        joined = [np.concatenate([p[j] for p in parts]) for j in range(5)]
        assert _same(whole[:5], joined), step
    with_start = dict(args, start=[3, 141, 7], kind=G.EMIT_COUNT, history_cap=G.state_cap(63) + 2)
    a = _ok(gm, 0, 65, **with_start)
    b = _ok(gm, 40, 25, **with_start)
    assert _same([x[40:] for x in a[:5]], b[:5])


def test_output_forms_chunks_and_a_second_call(gpu_lib, zoo_run):
    """NULL against requested outputs, device against host outputs, a workspace limit that forces chunks, a second call"""
    gm, args, whole = zoo_run
    bases, ln, fl, hist, hl, use = whole
    L, n = _ffi.lib(), 130
    only = _ok(gm, 0, n, 63, G.ENDABLE, None, 77, 0, False)
    assert _same((bases, ln, fl), only[:3]) and only[3] is None
    _ffi.check(L.phmm_sample_reads(gm._h, 0, n, 63, G.ENDABLE, None, 0, 77, None, None, None, None, 0, None, None))
    P = lambda x: x.ctypes.data_as(C.c_void_p)
    fl2 = np.zeros(n, dtype=np.uint32)
    _ffi.check(L.phmm_sample_reads(gm._h, 0, n, 63, G.ENDABLE, None, 0, 77, None, None, P(fl2), None, 66, None, None))
    assert np.array_equal(fl2, fl)
    db, dl, df = _DeviceArray(bases.nbytes, 0x55), _DeviceArray(ln.nbytes, 0x55), _DeviceArray(fl.nbytes, 0x55)
    dh, dhl, du = _DeviceArray(hist.nbytes, 0x55), _DeviceArray(hl.nbytes, 0x55), _DeviceArray(use.nbytes, 0x55)
    _ffi.check(L.phmm_sample_reads(gm._h, 0, n, 63, G.ENDABLE, None, 0, 77, db.p, dl.p, df.p, dh.p, 66, dhl.p, du.p))
    got = (db.numpy(np.uint8).reshape(bases.shape), dl.numpy(np.uint32), df.numpy(np.uint32),
           dh.numpy(np.uint32).reshape(hist.shape), dhl.numpy(np.uint32), du.numpy(np.uint32))
    assert _same(whole, got)
    second = _ok(gm, 0, n, **args)
    ws = gpu_lib.phmm_workspace_bytes()
    third = _ok(gm, 0, n, **args)
    assert gpu_lib.phmm_workspace_bytes() == ws and _same(whole, second) and _same(second, third)
    # per walk: staging rows of 64 bytes and 68 words, three words, and for host outputs dense rows of 64 bytes and 66 words
    per_walk = 64 + 4 * 68 + 12 + 64 + 4 * 66
    _ffi.check(gpu_lib.phmm_set_workspace_limit(256 + 4 * gm.n_nodes + 40 * per_walk))
    try:
        chunked = _ok(gm, 0, n, **args)
        launches = _ffi.last_call_stats(STATS)[1]
    finally:
        _ffi.check(gpu_lib.phmm_set_workspace_limit(0))
    assert launches == 4 and _same(whole, chunked)
    # no walks: nothing is written
    out = _ok(gm, 0, 0, **args)
    assert all(np.all(x == 0x77) or np.all(x == 0x77777777) for x in out)


def test_set_probs_to_other_numbers_and_back(gpu_lib):
    arrays = G.model("dbg")
    gm = D.PHMMModel(arrays)
    args = dict(length=40, kind=G.STATE_COUNT, seed=5, history_cap=41, usage=True)
    first = _ok(gm, 0, 70, **args)
    init2 = np.where(np.isfinite(arrays.init_logp), np.log(np.arange(1, arrays.n_nodes + 1) / 1e6), NINF)
    gm.set_probs(init2, arrays.trans_logp + math.log(0.5))
    other = _ok(gm, 0, 70, **args)
    a2 = D.PHMMArrays(arrays.param, arrays.emission, init2, arrays.edge_src, arrays.edge_dst, arrays.trans_logp + math.log(0.5))
    assert not np.array_equal(first[3], other[3]) and _same(other, _ok(D.PHMMModel(a2), 0, 70, **args))
    gm.set_probs(arrays.init_logp, arrays.trans_logp)
    assert _same(first, _ok(gm, 0, 70, **args))


# ------------------------------------------------------------------ 4. edges
def test_walks_that_run_off_a_linear_graph(models):
    gm = models["linear"]
    bases, ln, fl, hist, hl, _ = _ok(gm, 0, 64, 63, G.STATE_COUNT, None, 1, 65)
    assert np.all(fl == G.DEAD_END) and np.all(ln < 63) and np.all(ln > 0)
    assert all(hist[w, hl[w] - 1] == G.END for w in range(64))


def _big_model(init, prm=None):
    """100 000 nodes in a ring"""
    n = init.size
    v = np.arange(n, dtype=np.uint32)
    return D.PHMMArrays(prm or D.PHMMParams.uniform(0.01), np.frombuffer(b"ACGT" * (n // 4), dtype=np.uint8).copy(), init, v,
                        np.roll(v, -1), np.zeros(n))


def test_a_single_finite_init_among_100000_nodes(gpu_lib):
    init = np.full(100000, NINF)
    init[61803] = math.log(0.25)
    gm = D.PHMMModel(_big_model(init))
    bases, ln, fl, hist, hl, _ = _ok(gm, 0, 130, 2, G.STATE_COUNT, None, 9, 3)
    nodes = [x >> 2 for w in range(130) for x in hist[w].tolist() if x not in (G.INS_BEGIN, G.NONE)]
    firsts = [[x >> 2 for x in hist[w].tolist() if x not in (G.INS_BEGIN, G.NONE)][:1] for w in range(130)]
    assert sum(len(x) for x in firsts) >= 120 and all(x == [61803] for x in firsts if x) and not fl.any()
    assert set(nodes) <= {61803, 61804, 61805}


def test_every_init_at_minus_infinity(gpu_lib):
    gm = D.PHMMModel(_big_model(np.full(1000, NINF)))
    bases, ln, fl, hist, hl, use = _ok(gm, 0, 65, 10, G.EMIT_COUNT, None, 9, 4, True)
    assert np.all(fl == G.DEAD_END) and not ln.any() and not bases.any() and not use.any()
    assert np.all(hl == 1) and np.all(hist[:, 0] == G.END) and np.all(hist[:, 1:] == G.NONE)


def test_the_state_cap_returns(gpu_lib):
    """p_MM = p_MI = -inf and p_DD = 0 in logs on a cycle: a walk that enters Del never leaves it"""
    prm = D.PHMMParams.uniform(0.01).with_(p_MM=NINF, p_MI=NINF, p_MD=0.0, p_DD=0.0, p_DM=NINF, p_DI=NINF)
    gm = D.PHMMModel(_big_model(np.full(1000, math.log(1e-3)), prm))
    bases, ln, fl, hist, hl, _ = _ok(gm, 0, 65, 5, G.EMIT_COUNT, None, 9, 8)
    assert np.all(fl == (G.STATE_CAP | G.HISTORY_TRUNCATED)) and np.all(hl == G.state_cap(5)) and not ln.any()
    assert np.all(hist & 3 == G.DEL)


def test_endable_with_a_large_p_end_and_a_short_history_cap(models):
    arrays = G.model("zoo")
    gm = D.PHMMModel(D.PHMMArrays(arrays.param.with_(p_end=math.log(0.5)), arrays.emission, arrays.init_logp, arrays.edge_src,
                                  arrays.edge_dst, arrays.trans_logp))
    bases, ln, fl, hist, hl, _ = _ok(gm, 0, 130, 63, G.ENDABLE, None, 4, 65)
    # (a walk that starts near the end of the backbone may run off it before End is drawn)
    assert np.all((fl == G.ENDED) | (fl == G.DEAD_END)) and int((fl == G.ENDED).sum()) >= 120
    assert np.all(hl < 40) and all(hist[w, hl[w] - 1] == G.END for w in range(130))
    # the same walks with room for 3 words: the flag, and nothing else changes
    b2, ln2, fl2, hist2, hl2, _ = _ok(gm, 0, 130, 63, G.ENDABLE, None, 4, 3)
    assert np.array_equal(b2, bases) and np.array_equal(ln2, ln) and np.array_equal(hl2, hl)
    assert np.array_equal(fl2, fl | np.where(hl > 3, G.HISTORY_TRUNCATED, 0).astype(np.uint32)) and (hl > 3).any()
    assert np.array_equal(hist2, hist[:, :3])


def test_refusals(models):
    gm = models["zoo"]
    n = gm.n_nodes
    dead = int(np.flatnonzero(~np.isfinite(G.model("zoo").init_logp))[0])
    bad = [dict(length=0), dict(length=1 << 28), dict(kind=3), dict(start=[0, n]), dict(start=[dead, dead])]
    for kw in bad:
        a = dict(length=10, kind=0, start=None, seed=1, history_cap=11, usage=True)
        a.update(kw)
        length = a.pop("length")
        shape = length if 0 < length < 1000 else 10
        rc, *out = _raw_sized(gm, 4, length, shape, **a)
        assert rc == _ffi.PHMM_EINVAL, kw
        assert all(np.all(x == 0x77) or np.all(x == 0x77777777) for x in out), kw
    L = _ffi.lib()
    hist = np.full(8, 0x77777777, dtype=np.uint32)
    P = lambda x: x.ctypes.data_as(C.c_void_p)
    assert L.phmm_sample_reads(gm._h, 0, 2, 3, 0, None, 0, 1, None, None, None, P(hist), 0, None, None) == _ffi.PHMM_EINVAL
    assert L.phmm_sample_reads(gm._h, 0, 2, 3, 0, None, 2, 1, None, None, None, P(hist), 4, None, None) == _ffi.PHMM_EINVAL
    assert L.phmm_sample_reads(None, 0, 2, 3, 0, None, 0, 1, None, None, None, P(hist), 4, None, None) == _ffi.PHMM_EINVAL
    assert np.all(hist == 0x77777777)


def _raw_sized(gm, n, length, shape, kind, start, seed, history_cap, usage):
    """_raw with output arrays sized for `shape` where `length` itself is one the call refuses"""
    sn = None if start is None else np.ascontiguousarray(start, dtype=np.uint32)
    bases = np.full((n, shape + 1), 0x77, dtype=np.uint8)
    ln, fl, hl = (np.full(n, 0x77777777, dtype=np.uint32) for _ in range(3))
    hist = np.full((n, history_cap), 0x77777777, dtype=np.uint32)
    use = np.full(gm.n_nodes, 0x77777777, dtype=np.uint32)
    P = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
    rc = _ffi.lib().phmm_sample_reads(gm._h, 0, n, length, kind, P(sn), 0 if sn is None else sn.size, seed, P(bases), P(ln),
                                      P(fl), P(hist), history_cap, P(hl), P(use))
    return rc, bases, ln, fl, hist, hl, use


# ------------------------------------------------------------------ 5. the truth is a path of the forward model
def test_the_truth_is_a_path_of_the_forward_model(models):
    k = next(j for j, f in enumerate(G.fixtures()) if f["tag"].startswith("dbg kind 0 length 63"))
    f, gm = G.fixtures()[k], models["dbg"]
    bases, ln, fl, hist, hl, _ = _ok(gm, f["first_index"], f["n_walks"], f["length"], f["kind"], None, f["seed"], _cap(f))
    reads, lists, scores = [], [], []
    for w in range(f["n_walks"]):
        b = bases[w, :ln[w]].tobytes()
        t = G.truth(f["arrays"], hist[w, :hl[w]].tolist(), b)
        if t is None:
            continue
        value, n_terms, _ = B.score_path(f["arrays"], b, t[0], t[1])
        reads.append(b)
        lists.append(t[0])
        scores.append((value, n_terms))
    assert len(reads) >= 0.9 * f["n_walks"]
    rc = D.ReadCollection(reads)
    po, nd = B.csr(lists)
    mp = D.Mappings.from_arrays(rc, po, nd)
    best, _, _ = gm.run_with_mapping_best_path(rc, mp, want_path=False)
    _, full = gm.to_full_prob_reads(rc, mp)
    worst = 0.0
    for j, (value, n_terms) in enumerate(scores):
        bar = B.bar(n_terms + 4 * len(reads[j]), value)
        assert math.isfinite(value) and best[j] >= value - bar, (j, best[j], value)
        assert full[j] >= best[j] - bar, (j, full[j], best[j])
        worst = max(worst, best[j] - value)
    print(f"{len(reads)} of {f['n_walks']} walks have a truth; the best path beats it by at most {worst:.3f}")


# ------------------------------------------------------------------ 6. the wrapper
def _loop(walks, length, kind, n_reads=None, total_bases=None):
    """sample_by_profile's loop (sample.rs:198-235) over the restatement's walks in index order -> [(index, bases)]"""
    out, got = [], 0
    for i, (b, _, _, _) in enumerate(walks):
        if (n_reads is not None and len(out) >= n_reads) or (total_bases is not None and got >= total_bases):
            break
        if not b or (kind == G.EMIT_COUNT and len(b) != length):
            continue
        out.append((i, b))
        got += len(b)
    return out


def test_the_wrapper(models):
    gm, arrays = models["dbg"], G.model("dbg")
    for kind, name in ((G.STATE_COUNT, "state_count"), (G.EMIT_COUNT, "emit_count")):
        walks = [G.walk(arrays, 21, i, 30, kind) for i in range(60)]
        assert all(m >= G.MIN_MARGIN for _, _, _, m in walks)
        for amount in (dict(n_reads=17), dict(total_bases=400)):
            want = _loop(walks, 30, kind, **amount)
            assert want[-1][0] < 59
            results = [gm.sample_reads(30, name, seed=21, want_history=True, batch=batch, **amount) for batch in (1, 7, 4096)]
            for rc, info in results:
                assert rc.reads == [b for _, b in want] and info["walk_index"].tolist() == [i for i, _ in want]
                assert info["n_walks"] == want[-1][0] + 1
                assert [h.tolist() for h in info["history"]] == [walks[i][1] for i, _ in want]
                assert info["flags"].tolist() == [walks[i][2] for i, _ in want]
                if kind == G.EMIT_COUNT:
                    assert all(len(r) == 30 for r in rc.reads)
            if "total_bases" in amount:
                total = sum(len(b) for _, b in want)
                assert total >= 400 > total - len(want[-1][1])  # the read that crosses the total is kept
    rc, info = gm.sample_reads(60, n_reads=12, seed=2)
    mp, _ = gm.generate_mappings(rc)
    total, lp = gm.to_full_prob_reads(rc, mp)
    assert math.isfinite(total) and np.all(np.isfinite(lp))
