"""GPU: the tables of the list pass (phmm_run_with_mapping_tables, PHMMModel.run_with_mapping_tables):
forward_with_mapping (forward.rs:51-75) and backward_with_mapping (backward.rs:59-93) of every read on its lists, per
list entry ln m, i, d and per base the scalars of the column (ib, e forward; mb, ib backward), per read both totals.

Everything goes through the C ABI and is held, value by value, to the oracle's forward(read, FWD_MAPPING, lists) /
backward(read, BWD_MAPPING, lists), table(p), read at the listed nodes.

Bars (those of tests/test_gpu_states.py): a value whose oracle value lies within ln 1e-12 of the largest value of its
table at that position -- entries and scalars together -- is held at 1e-8; one below that floor must be -inf or below the
floor + 1e-8 on the GPU (a scaled column cannot hold more).  No value is left out.  Per-read totals 1e-9.

The parameters are not uniform, so that mb and ib of a backward table differ (a swap would pass otherwise)."""
import ctypes as C
import math

import numpy as np
import pytest

import caller_cases as cc
import dbgphmm_amd as D
from best_path_ref import pad_lists
from dbgphmm_amd import _ffi, _ffi_tables
from helpers import small_dbg_model, subset_csr
from repeat_cases import dataset

pytestmark = pytest.mark.gpu
LN_FLOOR = math.log(1e-12)
TOL = 1e-8
TOL_LOGP = 1e-9
STATS = 2  # index of phmm_last_call_stats the call fills
PARAM = D.PHMMParams.new(0.01, 0.02, 0.3, 1e-5, 40, 12)
NAMES = ("lf", "lb", "f", "fs", "b", "bs")


def _offsets(reads):
    off = np.zeros(len(reads) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    return off


def oracle_tables(oracle, arrays, reads, po, nd):
    """forward(read, FWD_MAPPING, its lists) / backward(read, BWD_MAPPING, its lists) of every read, table(p) at the listed
    nodes -> dict of the six arrays of the call   (restated from tests/test_list_tables_view_cpu.py)"""
    om = oracle.Model(arrays)
    off = _offsets(reads)
    po = po.astype(np.int64)
    te, tb = int(po[-1]), int(off[-1])
    out = {"f": np.full((te, 3), np.nan), "fs": np.full((tb, 2), np.nan), "b": np.full((te, 3), np.nan),
           "bs": np.full((tb, 2), np.nan), "lf": np.full(len(reads), np.nan), "lb": np.full(len(reads), np.nan)}
    for i, r in enumerate(reads):
        mp = oracle.Mapping(*subset_csr(off, (po.astype(np.uint64), nd, np.zeros(nd.size)), [i]))
        with np.errstate(divide="ignore"):
            F, B = om.forward(r, oracle.FWD_MAPPING, mp), om.backward(r, oracle.BWD_MAPPING, mp)
        for p in range(len(r)):
            g = off[i] + p
            v = nd[po[g]:po[g + 1]]
            for T, ent, scal, pick in ((F, out["f"], out["fs"], (1, 2)), (B, out["b"], out["bs"], (0, 1))):
                m, ins, d, s = T.table(p)
                ent[po[g]:po[g + 1], 0], ent[po[g]:po[g + 1], 1], ent[po[g]:po[g + 1], 2] = m[v], ins[v], d[v]
                scal[g] = s[pick[0]], s[pick[1]]
        out["lf"][i], out["lb"][i] = out["fs"][off[i + 1] - 1, 1], out["bs"][off[i], 0]
    assert not any(np.any(np.isnan(a)) for a in out.values())
    return out


def run(gm, rc, mp, want_forward=True, want_backward=True):
    """one call -> (dict of its arrays, (launches, cells) of the call)"""
    t = gm.run_with_mapping_tables(rc, mp, want_forward, want_backward)
    _, launches, cells = _ffi.last_call_stats(STATS)
    return {"lf": t.logp_forward, "lb": t.logp_backward, "f": t.fwd, "fs": t.fwd_scal, "b": t.bwd, "bs": t.bwd_scal, "t": t}, \
        (launches, cells)


def _same_bits(a, b, names=NAMES):
    return [k for k in names if not cc.same_bits(np.asarray(a[k]), np.asarray(b[k]))]


def _hold_table(what, po, ent, scal, ref_ent, ref_scal):
    """the bars of the module docstring for one table (forward or backward) over all positions"""
    po = po.astype(np.int64)
    n_pos = po.size - 1
    assert ent.shape == ref_ent.shape and scal.shape == ref_scal.shape == (n_pos, 2)
    assert not np.any(np.isnan(ent)) and not np.any(np.isnan(scal))
    cnt = np.diff(po)
    top = ref_scal.max(axis=1)
    if ref_ent.size:
        emax = np.full(n_pos, -np.inf)
        nz = cnt > 0
        emax[nz] = np.maximum.reduceat(ref_ent.max(axis=1), po[:-1][nz])
        top = np.maximum(top, emax)
    floor_e = np.repeat(top, cnt)[:, None] + LN_FLOOR
    floor_s = top[:, None] + LN_FLOOR
    worst, n_low = 0.0, 0
    for got, ref, floor in ((ent, ref_ent, floor_e), (scal, ref_scal, floor_s)):
        floor = np.broadcast_to(floor, ref.shape)
        hi = ref >= floor
        with np.errstate(invalid="ignore"):
            d = np.where(got == ref, 0.0, np.abs(got - ref))  # (-inf against -inf is a match)
        assert not np.any(np.isnan(d[hi])), what + ": a value the oracle holds finite is -inf (or the reverse)"
        if np.any(hi):
            worst = max(worst, float(d[hi].max()))
        low = ~hi
        n_low += int(low.sum())
        assert np.all((got[low] == -np.inf) | (got[low] < floor[low] + TOL)), what + ": a value under the floor is too large"
    print(f"{what}: worst |d| {worst:.3e} (bound {TOL:.0e}), {n_low} values under the floor")
    assert worst <= TOL
    return worst


def _hold(what, po, got, ref):
    _hold_table(what + ", forward", po, got["f"], got["fs"], ref["f"], ref["fs"])
    _hold_table(what + ", backward", po, got["b"], got["bs"], ref["b"], ref["bs"])
    for k in ("lf", "lb"):
        with np.errstate(invalid="ignore"):
            d = np.where(got[k] == ref[k], 0.0, np.abs(got[k] - ref[k]))
        print(f"{what}: max |d {k}| {float(d.max()):.3e} (bound {TOL_LOGP:.0e})")
        assert not np.any(np.isnan(d)) and float(d.max()) <= TOL_LOGP


def _totals_are_the_scalars(rc, got):
    off = rc.offsets.astype(np.int64)
    for r in range(len(rc)):
        if off[r + 1] > off[r]:
            assert cc.same_bits(got["lf"][r:r + 1], got["fs"][off[r + 1] - 1, 1:2]), r
            assert cc.same_bits(got["lb"][r:r + 1], got["bs"][off[r], 0:1]), r


# ------------------------------------------------------------------ the fixture
@pytest.fixture(scope="module")
def base(oracle):
    """a 500-base diploid genome at k = 12 (more than 400 nodes: a list can be padded to 400), four reads of about 100
    bases and their prefixes of 1 and 2 bases, the oracle's own lists per n_max_gaps: at most 64 nodes for the long reads,
    400 at every base of the two short ones (they end inside the oracle's dense warm-up), so a call has both classes"""
    hap = D.random_genome(500, 31)
    sg = D.dbg_from_haplotypes([hap, D.diverge(hap, 0.02, 32)], 12)
    arrays = {g: D.vectorised_to_phmm(sg, PARAM.with_(n_max_gaps=g), 0) for g in (0, 4, 6)}
    assert arrays[4].n_nodes > 410
    reads = [r for r in D.sample_reads(arrays[4], 10 ** 9, 100, seed=33, max_reads=16) if len(r) >= 90][:4]
    assert len(reads) == 4 and all(len(r) <= 110 for r in reads)
    reads = reads + [reads[0][:1], reads[1][:2]]
    lists = {}
    for g in (0, 4, 6):
        (po, nd, _), _ = oracle.Model(arrays[g]).generate_mappings(reads, None, True, n_threads=4)
        lists[g] = (po, nd)
    return sg, arrays, reads, lists


_ref_cache = {}


def _case(oracle, base, gaps, width):
    """(arrays, reads, (po, nd), the oracle's tables) of one parity case; computed once, shared, left unchanged"""
    sg, arrays, reads, lists = base
    key = (gaps, width)
    if key not in _ref_cache:
        po, nd = lists[gaps]
        if width is not None:
            po, nd = pad_lists(po, nd, reads, arrays[gaps].n_nodes, width)
        _ref_cache[key] = ((po, nd), oracle_tables(oracle, arrays[gaps], reads, po, nd))
    return arrays[gaps], reads, _ref_cache[key][0], _ref_cache[key][1]


# ------------------------------------------------------------------ 1. parity of all six outputs
@pytest.mark.parametrize("width", [None, 64, 65, 400], ids=["as_generated", "pad64", "pad65", "pad400"])
@pytest.mark.parametrize("gaps", [0, 4, 6])
def test_parity_of_all_six_outputs(gpu_lib, oracle, base, gaps, width):
    """Fails without the feature: the call does not exist."""
    arrays, reads, (po, nd), ref = _case(oracle, base, gaps, width)
    cnt, off = np.diff(po.astype(np.int64)), _offsets(reads)
    longest = int(cnt[:off[4]].max())  # of the four long reads; the two short ones have lists of 400 throughout
    assert (longest == width if width is not None else longest <= 64) and np.all(cnt[off[4]:] == 400)
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    mp = D.Mappings.from_arrays(rc, po, nd)
    got, (launches, cells) = run(gm, rc, mp)
    what = f"n_max_gaps {gaps}, longest list of the long reads {longest}"
    _hold(what, po, got, ref)
    _totals_are_the_scalars(rc, got)
    assert cells == int(po[-1]) and launches >= 2
    # mb and ib of the backward tables differ: the bars above would see a swap
    assert np.median(np.abs(ref["bs"][:, 0] - ref["bs"][:, 1])) > 0.2
    lf_states, _, _ = gm.run_with_mapping_states(rc, mp, want_states=False, want_best=False)
    d = float(np.max(np.abs(got["lf"] - lf_states)))
    print(f"{what}: max |ln P - the states call's| {d:.3e}")
    assert d <= TOL_LOGP


# ------------------------------------------------------------------ 2. halves
@pytest.mark.parametrize("width", [None, 65], ids=["as_generated", "pad65"])
def test_halves_return_the_bits_of_the_full_call(gpu_lib, oracle, base, width):
    arrays, reads, (po, nd), _ = _case(oracle, base, 4, width)
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    mp = D.Mappings.from_arrays(rc, po, nd)
    full, st_full = run(gm, rc, mp)
    fwd, st_f = run(gm, rc, mp, want_backward=False)
    bwd, st_b = run(gm, rc, mp, want_forward=False)
    assert all(fwd[k] is None for k in ("lb", "b", "bs")) and all(bwd[k] is None for k in ("lf", "f", "fs"))
    assert not _same_bits(full, fwd, ("lf", "f", "fs")) and not _same_bits(full, bwd, ("lb", "b", "bs"))
    print(f"(launches, cells): full {st_full}, forward only {st_f}, backward only {st_b}")
    assert 0 < st_f[0] < st_full[0] and 0 < st_b[0] < st_full[0] and st_f[0] + st_b[0] == st_full[0]
    # nothing asked for: nothing is run
    _ffi.check(_ffi_tables.lib().phmm_run_with_mapping_tables(gm._h, rc._h, mp._h, None, None, None, None, None, None))
    assert _ffi.last_call_stats(STATS)[1] == 0
    # the scalars alone, the totals alone: the same bits again
    fs, bs, lf, lb = np.empty((rc.total_bases(), 2)), np.empty((rc.total_bases(), 2)), np.empty(len(rc)), np.empty(len(rc))
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    _ffi.check(_ffi_tables.lib().phmm_run_with_mapping_tables(gm._h, rc._h, mp._h, None, None, None, P(fs), None, P(bs)))
    _ffi.check(_ffi_tables.lib().phmm_run_with_mapping_tables(gm._h, rc._h, mp._h, P(lf), P(lb), None, None, None, None))
    assert cc.same_bits(fs, full["fs"]) and cc.same_bits(bs, full["bs"])
    assert cc.same_bits(lf, full["lf"]) and cc.same_bits(lb, full["lb"])


# ------------------------------------------------------------------ 3. holes
def _with_lists(po, nd, reads, change):
    """the CSR with change(read, pos, own list) -> new list applied to every position"""
    out_off, out, g = [0], [], 0
    for i, r in enumerate(reads):
        for p in range(len(r)):
            lst = np.asarray(change(i, p, nd[int(po[g]):int(po[g + 1])]), dtype=np.uint32)
            out.append(lst)
            out_off.append(out_off[-1] + lst.size)
            g += 1
    return np.array(out_off, np.uint64), np.concatenate(out).astype(np.uint32)


def test_holes_are_results(gpu_lib, oracle, base):
    """read 0: the list of base 50 emptied (e = -inf there, the InsBegin chain carries on and re-enters); read 1: the list
    of base 40 replaced by nodes that are neither children of list 39 nor parents of list 41"""
    sg, arrays_by, reads, lists = base
    arrays = arrays_by[4]
    po, nd = lists[4]
    off = _offsets(reads)
    src, dst = arrays.edge_src, arrays.edge_dst
    before = nd[int(po[off[1] + 39]):int(po[off[1] + 40])]
    after = nd[int(po[off[1] + 41]):int(po[off[1] + 42])]
    linked = np.concatenate([dst[np.isin(src, before)], src[np.isin(dst, after)], before, after,
                             nd[int(po[off[1] + 40]):int(po[off[1] + 41])]])
    apart = np.setdiff1d(np.arange(arrays.n_nodes, dtype=np.uint32), linked)[:5]
    assert apart.size == 5

    def change(i, p, own):
        if i == 0 and p == 50:
            return own[:0]
        if i == 1 and p == 40:
            return apart
        return own

    hpo, hnd = _with_lists(po, nd, reads, change)
    ref = oracle_tables(oracle, arrays, reads, hpo, hnd)
    g0 = int(off[0]) + 50
    assert ref["fs"][g0, 1] == -np.inf and np.isfinite(ref["fs"][g0 + 2, 1])  # the oracle: e = -inf, finite again behind
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    got, _ = run(gm, rc, D.Mappings.from_arrays(rc, hpo, hnd))
    _hold("holes", hpo, got, ref)
    _totals_are_the_scalars(rc, got)
    assert got["fs"][g0, 1] == -np.inf
    for k in ("f", "fs", "b", "bs"):  # the oracle's -inf is -inf here
        assert np.all(got[k][ref[k] == -np.inf] == -np.inf), k
    print(f"holes: ln P forward {got['lf'][:2]}, the oracle's {ref['lf'][:2]}")


def test_a_read_of_probability_zero_is_a_result(gpu_lib, oracle, base):
    """the nodes of read 0's last list go to copy number 0: its last column is dead, ln P = -inf forward and backward, and
    the call returns it (the states call refuses such a read set)"""
    sg, arrays_by, reads, lists = base
    po, nd = lists[4]
    off = _offsets(reads)
    dead = nd[int(po[off[1] - 1]):int(po[off[1]])]
    cn = sg.copy_num.copy()
    cn[dead] = 0
    with np.errstate(divide="ignore"):
        arrays = D.vectorised_to_phmm(D.SeqGraph(cn, sg.base, sg.edge_src, sg.edge_dst, None), PARAM, 0)
        ref = oracle_tables(oracle, arrays, reads, po, nd)
    assert ref["lf"][0] == -np.inf and ref["lb"][0] == -np.inf and np.isfinite(ref["lf"][2])
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    got, _ = run(gm, rc, D.Mappings.from_arrays(rc, po, nd))
    _hold("probability 0", po, got, ref)
    assert got["lf"][0] == -np.inf and got["lb"][0] == -np.inf
    assert np.all(got["t"].ins_begin_posterior(0) == -np.inf)


# ------------------------------------------------------------------ 4. the cut read
def test_cut_read_scalar_tracks_and_the_ins_begin_posterior(gpu_lib, oracle):
    """the case of tests/test_oracle_edge_semantics.py: a 900-base genome, reads of about 400 bases, the best node of base
    300 of read 0 at copy number 0.  The oracle gives an InsBegin posterior of 0.997 over bases 0..298, 0.988 at 299 and
    6e-32 at 310."""
    arrays, sg = small_dbg_model(900, 12, 0.003, seed=21)
    reads = [r for r in D.sample_reads(arrays, 10 ** 9, 420, seed=22, max_reads=40) if len(r) > 380][:2]
    (po, nd, _), _ = oracle.Model(arrays).generate_mappings(reads, None, True, n_threads=4)
    cut_at = 300
    cn = sg.copy_num.copy()
    cn[int(nd[int(po[cut_at])])] = 0
    with np.errstate(divide="ignore"):
        a1 = D.vectorised_to_phmm(D.SeqGraph(cn, sg.base, sg.edge_src, sg.edge_dst, None), arrays.param, 0)
        ref = oracle_tables(oracle, a1, reads, po, nd)
    assert np.all(np.isfinite(ref["lf"]))
    gm, rc = D.PHMMModel(a1), D.ReadCollection(reads)
    got, _ = run(gm, rc, D.Mappings.from_arrays(rc, po, nd))
    # both scalar tracks under the bars (the floor of a position from its whole table, entries included)
    _hold("cut read", po, got, ref)
    _totals_are_the_scalars(rc, got)
    post = got["t"].ins_begin_posterior(0)
    want = D.ListTables.from_arrays(rc.offsets, po, nd, a1.param.p_end, a1.n_nodes, ref["f"], ref["fs"], ref["b"],
                                    ref["bs"]).ins_begin_posterior(0)
    print(f"cut read: InsBegin posterior at bases 0, 298, 299, 310: {np.exp(post[[0, 298, 299, 310]])}, "
          f"the oracle's {np.exp(want[[0, 298, 299, 310]])}; ln P {got['lf'][0]:.3f} / {ref['lf'][0]:.3f}")
    assert np.all(np.exp(post[:cut_at - 1]) > 0.9)
    assert np.exp(post[cut_at + 10]) < 1e-6
    assert np.max(np.abs(post[:cut_at] - want[:cut_at])) < 1e-7


# ------------------------------------------------------------------ 5. refusals
def _status(fn):
    try:
        fn()
    except D.PhmmError as e:
        return e.code
    return _ffi.PHMM_OK


class _Prefilled:
    """outputs of a raw call, pre-filled: a refusal leaves them as they are"""

    def __init__(self, n_reads, bases, entries):
        self.a = [np.full(n_reads, 7.5), np.full(n_reads, 7.5), np.full((max(entries, 1), 3), 7.5),
                  np.full((max(bases, 1), 2), 7.5), np.full((max(entries, 1), 3), 7.5), np.full((max(bases, 1), 2), 7.5)]

    def call(self, gm, rc, mp):
        _ffi.check(_ffi_tables.lib().phmm_run_with_mapping_tables(gm._h, rc._h, mp._h,
                                                                  *[a.ctypes.data_as(C.c_void_p) for a in self.a]))

    def untouched(self):
        return all(bool(np.all(a == 7.5)) for a in self.a)


def test_refusals(gpu_lib, base):
    sg, arrays_by, reads, lists = base
    arrays = arrays_by[4]
    po, nd = lists[4]
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    mp = D.Mappings.from_arrays(rc, po, nd)
    rc2 = D.ReadCollection(reads[:2])
    n = len(reads[0]) + len(reads[1])
    # a list of 401 nodes (refused where the lists are handed over, as for the states call)
    def list_of_401(call):
        over = D.Mappings.from_arrays(rc2, np.arange(n + 1, dtype=np.uint64) * 401, np.tile(np.arange(401, dtype=np.uint32), n))
        call(gm, rc2, over)

    out = _Prefilled(2, n, 401 * n)
    assert _status(lambda: list_of_401(out.call)) == _ffi.PHMM_ECAPACITY and out.untouched()
    # mappings of another read set
    out = _Prefilled(2, n, int(po[-1]))
    assert _status(lambda: out.call(gm, rc2, mp)) == _ffi.PHMM_EINVAL and out.untouched()
    # a node twice in one list: found on the device, by either half
    dpo, dnd = _with_lists(po, nd, reads, lambda i, p, own: np.concatenate([own, own[:1]]) if (i, p) == (2, 30) else own)
    dup = D.Mappings.from_arrays(rc, dpo, dnd)
    for wf, wb in ((True, True), (True, False), (False, True)):
        assert _status(lambda: gm.run_with_mapping_tables(rc, dup, wf, wb)) == _ffi.PHMM_EINVAL, (wf, wb)
    # NULL handles
    L = _ffi_tables.lib()
    assert L.phmm_run_with_mapping_tables(None, rc._h, mp._h, None, None, None, None, None, None) == _ffi.PHMM_EINVAL
    assert L.phmm_run_with_mapping_tables(gm._h, None, mp._h, None, None, None, None, None, None) == _ffi.PHMM_EINVAL
    assert L.phmm_run_with_mapping_tables(gm._h, rc._h, None, None, None, None, None, None, None) == _ffi.PHMM_EINVAL
    # no reads: nothing is written
    rc0 = D.ReadCollection([])
    mp0 = D.Mappings.from_arrays(rc0, np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint32))
    out = _Prefilled(1, 0, 0)
    out.call(gm, rc0, mp0)
    assert out.untouched()
    # and the call still works
    run(gm, rc, mp)


# ------------------------------------------------------------------ 6. wide lists from a real repeat
def test_wide_lists_from_a_real_repeat(gpu_lib, oracle):
    arrays, reads, _, _ = dataset("u20n200", 40, max_reads=3)
    reads = [r[:300] for r in reads]
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    mp, _ = gm.generate_mappings(rc, None, True)
    po, nd, _ = mp.arrays()
    cnt = np.diff(po.astype(np.int64))
    off = rc.offsets.astype(np.int64)
    rmax = [int(cnt[off[r]:off[r + 1]].max()) for r in range(len(rc))]
    print(f"u20n200: longest list per read {rmax}")
    assert all(64 < m <= 400 for m in rmax)
    ref = oracle_tables(oracle, arrays, reads, po, nd)
    got, (launches, cells) = run(gm, rc, mp)
    _hold("u20n200", po, got, ref)
    _totals_are_the_scalars(rc, got)
    assert cells == int(po[-1])


# ------------------------------------------------------------------ 7. chunks
def test_chunks_return_the_unlimited_bits(gpu_lib, oracle, base):
    """a chunk is two to four launches (a forward and a backward one per class it holds): nine launches or more are three
    chunks or more"""
    arrays, reads, (po, nd), _ = _case(oracle, base, 4, None)
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    mp = D.Mappings.from_arrays(rc, po, nd)
    whole, (launches, _) = run(gm, rc, mp)
    assert launches == 4  # both classes, both halves, one chunk
    staged = 48 * int(po[-1]) + 32 * rc.total_bases()
    _ffi.check(gpu_lib.phmm_set_workspace_limit(staged // 3))
    try:
        parts, (launches, cells) = run(gm, rc, mp)
    finally:
        _ffi.check(gpu_lib.phmm_set_workspace_limit(0))
    print(f"chunks: {launches} launches under a limit of {staged // 3} bytes")
    assert launches >= 9 and cells == int(po[-1])
    assert not _same_bits(whole, parts)


# ------------------------------------------------------------------ 8. the caller contract
@pytest.fixture(scope="module")
def ctx(gpu_lib):
    return cc.Ctx()


@pytest.fixture(scope="module")
def scratch(gpu_lib):
    s = cc.DeviceArray(cc.SCRATCH_BYTES, 0)
    yield s
    s.free()


def _row():
    """the new entry point as a row of caller_cases"""
    TL = _ffi_tables.lib()
    outs = lambda c: [cc.Out("logp_forward", cc.F8, (c.R,)), cc.Out("logp_backward", cc.F8, (c.R,)),  # noqa: E731
                      cc.Out("forward", cc.F8, (c.entries, 3)), cc.Out("forward_scalars", cc.F8, (c.bases, 2)),
                      cc.Out("backward", cc.F8, (c.entries, 3)), cc.Out("backward_scalars", cc.F8, (c.bases, 2))]

    def call(c, b):
        c.ffi.check(TL.phmm_run_with_mapping_tables(c.gm._h, c.rc._h, c.mp._h, b["logp_forward"], b["logp_backward"],
                                                    b["forward"], b["forward_scalars"], b["backward"], b["backward_scalars"]))
    return cc.Row("run_with_mapping_tables", list(_ffi_tables.TABLES_SYMBOLS["phmm_amd_tables.h"]), outs, call)


def test_device_outputs_and_a_busy_stream(ctx, scratch):
    """every output into poisoned device buffers: the host form's bits and nothing behind an output's extent; then the
    same on a hipStreamNonBlocking stream that is still busy when the call starts; then a mix of host, device and NULL"""
    row = _row()
    want = cc.run_host(ctx, row)
    assert np.all(np.isfinite(want["logp_forward"])) and not np.any(np.isnan(want["forward"]))
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
    # the entries on the device, the scalars on the host, no totals
    d = cc.DeviceOutputs(ctx, row)
    try:
        ptrs = d.pointers()
        host = {k: np.zeros_like(want[k]) for k in ("forward_scalars", "backward_scalars")}
        ptrs.update({k: v.ctypes.data_as(C.c_void_p) for k, v in host.items()})
        ptrs.update(logp_forward=None, logp_backward=None)
        row.call(ctx, ptrs)
        got, clean = d.read()
        assert clean and cc.same_bits(got["forward"], want["forward"]) and cc.same_bits(got["backward"], want["backward"])
        assert all(cc.same_bits(host[k], want[k]) for k in host)
        assert np.all(got["logp_forward"].view(np.uint8) == cc.POISON)
    finally:
        d.free()


def test_four_calls_do_not_grow_the_workspace(ctx):
    row = _row()
    runs, ws = [], []
    for _ in range(4):
        runs.append(cc.run_host(ctx, row))
        ws.append(ctx.lib.phmm_workspace_bytes())
    assert ws[1] == ws[2] == ws[3], ws
    for k in (1, 2, 3):
        assert not cc.same_result(runs[0], runs[k]), (k, cc.same_result(runs[0], runs[k]))
