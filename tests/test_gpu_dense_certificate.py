"""GPU: the dense certificate (exact_dense.hip: certify_dense) swept across its threshold.

The scaled linear kernels flush a cell more than ~700 nats below its column maximum; the certificate flags the reads
for which such cells could matter, and those are recomputed in log space.  A detector that passes a read it should
have flagged gives a finite, plausible, wrong ln P, so the reads here are placed ON the threshold: chimeras
A[:a] + B[:a + 80] of two sampled reads, whose second half aligns where the first half made it ever less likely as
`a` grows.  The depth proxy of a read is taken from the oracle's tables: the largest value over the columns of
(column maximum of F) - (largest F among the cells whose F + B lies within 1 nat of ln P), i.e. how far below the
column maximum the cells that end up carrying the read have been.  By the certificate's own constants it flags from
about 1022 - 64 - 50 - log2(6 N len) ~ 885 bits ~ 615 nats on; the scaled values are gone at 708-745 nats.

PHMM_NO_EXACT_DENSE=1 shows what the certificate decided: a flagged read comes back NaN and its posteriors are left
out of the sums, so every read that is NOT NaN has to meet the fast path's own bar (1e-9) against the oracle.  The
mirrored family B[:s + 80] + A[:s] does the same to the backward half.  The batch (> 64 reads, ordinary reads in
between) also runs the fallback's bookkeeping with flagged reads in several groups and chunks."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import dbgphmm_amd as D
from dbgphmm_amd import _ffi
from helpers import finite_close, small_dbg_model

pytestmark = pytest.mark.gpu

FWD_A = tuple(range(100, 293, 8))    # 25 reads
MIR_S = tuple(range(100, 293, 24))   # 9 reads
TOL_FAST = 1e-9    # the dense bar (test_gpu_dense.py: TOL_LOGP)
TOL_FREQ = 1e-8
TOL_EXACT = 1e-6   # the bar the exact path is pinned at (test_chimeric_read_takes_the_exact_path)
SHALLOW, DEEP = 400.0, 800.0


class _env:
    """environment knobs for the calls inside the block (knobs are read when a call takes the device)"""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.before = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.before.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _knobs(switch, w):
    return _env(PHMM_NO_EXACT_DENSE="1" if switch else None, PHMM_DENSE_W=w)


def depth_proxy(out):
    """-> (F depth, B depth, F depth same-index, B depth same-index).  T depth: max over the merged columns i = 1 .. L
    (F.tables[i-1] with B.tables[i], b_init = p_end at i = L: the pairing of the posteriors, table.rs:414-434, 500-505)
    of max(T) - max(T over the cells with F + B >= ln P - 1).  The same-index values pair F.tables[i] with B.tables[i]
    instead, which counts x[i] twice and so meets the bound only where the path repeats a base: they see a quarter of
    the columns and come out lower (see `shallow` in build_family for their use)."""
    L = len(out.read)
    P = out.to_full_prob_forward()
    p_end = out.model.param.p_end
    worst = [0.0, 0.0, 0.0, 0.0]
    f_prev = None
    for i in range(L + 1):
        f = np.concatenate(out.forward.table(i)[:3]) if i < L else None
        b = np.concatenate(out.backward.table(i)[:3]) if i < L else np.full(f_prev.size, p_end)
        for slot, ff in ((0, f_prev), (2, f)):
            if ff is None:
                continue
            with np.errstate(invalid="ignore"):
                on = (ff + b) >= P - 1.0
            if on.any():
                worst[slot] = max(worst[slot], float(ff.max() - ff[on].max()))
                worst[slot + 1] = max(worst[slot + 1], float(b.max() - b[on].max()))
        f_prev = f
    return tuple(worst)


class Family:
    pass


def build_family(oracle):
    fam = Family()
    arrays, _ = small_dbg_model(500, 12, 0.01, seed=17, min_copy_num=1)
    assert arrays.n_nodes == 637
    src = [r for r in D.sample_reads(arrays, 10 ** 9, 400, seed=9, max_reads=60) if len(r) >= 330][:2]
    A, B = src
    fwd = [A[:a] + B[:a + 80] for a in FWD_A]
    mir = [B[:s + 80] + A[:s] for s in MIR_S]
    plain = D.sample_reads(arrays, 10 ** 9, 150, seed=3, max_reads=41)
    plain = [r[:max(30, len(r) - (j * 7) % 121)] for j, r in enumerate(plain) if len(r) >= 30]
    assert len(plain) >= 36 and all(30 <= len(r) <= 150 for r in plain)
    # interleave: chimeras at every other slot while they last
    chim = [("fwd", j, r) for j, r in enumerate(fwd)] + [("mir", j, r) for j, r in enumerate(mir)]
    reads, kind = [], []
    for j in range(max(len(chim), len(plain))):
        if j < len(plain):
            reads.append(plain[j])
            kind.append(("plain", j))
        if j < len(chim):
            reads.append(chim[j][2])
            kind.append(chim[j][:2])
    assert len(reads) > 64
    om = oracle.Model(arrays)
    R = len(reads)
    fam.arrays, fam.om, fam.reads, fam.kind = arrays, om, reads, kind
    fam.lf, fam.lb, fam.proxies = np.empty(R), np.empty(R), np.zeros((R, 4))
    fam.nf, fam.ef, fam.inf = np.empty((R, arrays.n_nodes)), np.empty((R, arrays.n_edges)), np.empty((R, arrays.n_nodes))

    def one(r):
        o = om.run(reads[r])
        fam.lf[r], fam.lb[r] = o.to_full_prob_forward(), o.to_full_prob_backward()
        fam.nf[r] = o.to_node_freqs()
        fam.ef[r], fam.inf[r] = o.to_edge_and_init_freqs()
        if kind[r][0] != "plain":
            fam.proxies[r] = depth_proxy(o)

    with ThreadPoolExecutor(8) as pool:  # (the oracle's calls release the interpreter lock)
        list(pool.map(one, range(R)))
    fam.is_fwd = np.array([k[0] == "fwd" for k in kind])
    fam.is_mir = np.array([k[0] == "mir" for k in kind])
    fam.is_plain = np.array([k[0] == "plain" for k in kind])
    fam.a = np.array([FWD_A[k[1]] if k[0] == "fwd" else (MIR_S[k[1]] if k[0] == "mir" else 0) for k in kind])
    # The family's own proxy: on F for the forward family, on B for the mirrored one.  A read is flagged by either half
    # of the certificate, so what must not be flagged is a read shallow on BOTH sides: the mirrored reads s = 268 and 292
    # are 163 and 214 nats deep on B and 1029 and 1143 on F (their best placement flips to the A half), and are flagged.
    # For the forward family the same-index pairing adds a = 156 and 164 to that set; for the mirrored one it is no
    # measure (s = 220: 345 nats where the posterior pairing gives 689, past the ~615 the certificate flags from).
    dF, dB, dF_same, dB_same = fam.proxies.T
    fam.depth = np.where(fam.is_mir, dB, dF)
    fam.depth_same = np.where(fam.is_mir, dB_same, dF_same)
    fam.depth_both = np.maximum(dF, dB)
    fam.shallow = ~fam.is_plain & ((fam.depth_both < SHALLOW) | (fam.is_fwd & (np.maximum(dF_same, dB_same) < SHALLOW)))
    return fam


@pytest.fixture(scope="module")
def family(oracle):
    fam = build_family(oracle)
    for name, depth in (("posterior pairing", fam.depth), ("same-index pairing", fam.depth_same)):
        d = depth[fam.is_fwd]
        print(f"{name}: forward family a {fam.a[fam.is_fwd].tolist()} depth (nats) {np.round(d, 1).tolist()}")
        print(f"{name}: mirrored family s {fam.a[fam.is_mir].tolist()} depth on B (nats) {np.round(depth[fam.is_mir], 1).tolist()}")
        # conditions on the inputs: reads on both sides of the threshold and no hole where it lies
        assert (d < SHALLOW).sum() >= 5 and (d > DEEP).sum() >= 5
        band = np.sort(d[(d >= 485.0) & (d <= 735.0)])
        assert band.size >= 2 and np.max(np.diff(np.concatenate([[485.0], band, [735.0]]))) <= 60.0, band
    print(f"mirrored family, depth on F (nats) {np.round(fam.proxies[fam.is_mir, 0], 1).tolist()}")
    assert fam.shallow[fam.is_fwd].sum() >= 5 and fam.shallow[fam.is_mir].sum() >= 3
    return fam


def _call(gm, rc):
    lf, lb, nf = gm.run_dense(rc)
    lf_e, ef, inf = gm.run_dense_edge_freqs(rc)
    lf_o, _, _ = gm.run_dense(rc, False, False)
    return dict(lf=lf, lb=lb, nf=nf, lf_e=lf_e, ef=ef, inf=inf, lf_o=lf_o)


def _dev(got, want, sel):
    with np.errstate(invalid="ignore"):
        return float(np.max(np.abs(got[sel] - want[sel]), initial=0.0))


@pytest.fixture(scope="module")
def handles(gpu_lib, family):
    return D.PHMMModel(family.arrays), D.ReadCollection(family.reads)


@pytest.fixture(scope="module")
def switched(handles):
    """the batch under PHMM_NO_EXACT_DENSE=1 at the automatic group width: what the certificate decided"""
    gm, rc = handles
    with _knobs(True, None):
        return _call(gm, rc)


def _check_soundness(fam, res, label):
    nan = np.isnan(res["lf"])
    assert np.array_equal(nan, np.isnan(res["lb"])) and np.array_equal(nan, np.isnan(res["lf_e"]))
    ok = ~nan
    d_lf, d_lb, d_e = _dev(res["lf"], fam.lf, ok), _dev(res["lb"], fam.lb, ok), _dev(res["lf_e"], fam.lf, ok)
    d_nf = float(np.max(np.abs(res["nf"] - fam.nf[ok].sum(axis=0))))
    d_ef = float(np.max(np.abs(res["ef"] - fam.ef[ok].sum(axis=0))))
    d_if = float(np.max(np.abs(res["inf"] - fam.inf[ok].sum(axis=0))))
    flagged_a = sorted(fam.a[nan & fam.is_fwd].tolist())
    print(f"{label}: flagged forward a {flagged_a}, mirrored s {sorted(fam.a[nan & fam.is_mir].tolist())}; "
          f"shallowest flagged depth (either side) {np.min(fam.depth_both[nan], initial=np.inf):.1f} nats, deepest passed "
          f"{np.max(fam.depth_both[ok]):.1f}; unflagged reads: max |d lf| {d_lf:.3e} |d lb| {d_lb:.3e} (edge call {d_e:.3e}) "
          f"nf {d_nf:.3e} ef {d_ef:.3e} if {d_if:.3e}")
    assert d_lf <= TOL_FAST and d_lb <= TOL_FAST and d_e <= TOL_FAST
    assert d_nf <= TOL_FREQ and d_ef <= TOL_FREQ and d_if <= TOL_FREQ
    n_fwd = int((nan & fam.is_fwd).sum())
    assert 0 < n_fwd < int(fam.is_fwd.sum())
    assert not (nan & fam.is_plain).any()
    assert not (nan & fam.shallow).any()
    # forward-only call: the second look with fetched backward maxima
    nan_o = np.isnan(res["lf_o"])
    d_o = _dev(res["lf_o"], fam.lf, ~nan_o)
    print(f"{label}: forward-only call flags {int(nan_o.sum())} of the {int(nan.sum())}; max |d lf| {d_o:.3e}")
    assert d_o <= TOL_FAST
    assert not (nan_o & ~nan).any()
    return nan


@pytest.mark.parametrize("w", [None, "8"])
def test_unflagged_reads_meet_the_fast_bar(handles, family, switched, w):
    gm, rc = handles
    if w is None:
        res = switched
    else:
        with _knobs(True, w):
            res = _call(gm, rc)
    nan = _check_soundness(family, res, f"switch on, W {w or 'auto'}")
    assert np.array_equal(nan, np.isnan(switched["lf"]))  # the decision is per read, whatever the grouping


@pytest.mark.parametrize("w", [None, "8"])
def test_default_path_equals_the_oracle(handles, family, switched, w):
    fam = family
    gm, rc = handles
    with _knobs(False, w):
        res = _call(gm, rc)
    every = np.ones(len(fam.reads), bool)
    for k in ("lf", "lb", "lf_e", "lf_o", "nf", "ef", "inf"):
        assert np.all(np.isfinite(res[k])), k
    assert (fam.lf[fam.is_fwd & (fam.a >= 204)] < -709.0).all()  # below the range of exp: finite all the same
    shallow = fam.shallow
    was_nan = np.isnan(switched["lf"])
    for k, want in (("lf", fam.lf), ("lb", fam.lb), ("lf_e", fam.lf), ("lf_o", fam.lf)):
        print(f"default, W {w or 'auto'}: {k}: max dev all {_dev(res[k], want, every):.3e}, shallow "
              f"{_dev(res[k], want, shallow):.3e}, reads flagged under the switch {_dev(res[k], want, was_nan):.3e}")
        assert _dev(res[k], want, every) <= TOL_EXACT, k
        assert _dev(res[k], want, shallow) <= TOL_FAST, k
    for k, want in (("nf", fam.nf), ("ef", fam.ef), ("inf", fam.inf)):
        d = float(np.max(np.abs(res[k] - want.sum(axis=0))))
        print(f"default, W {w or 'auto'}: {k}: max dev {d:.3e}")
        assert d <= TOL_EXACT, k


@pytest.mark.parametrize("switch", [False, True])
def test_chunked_workspace(gpu_lib, handles, family, switch):
    """W = 8 under a workspace limit of one group per chunk: flagged reads in the first chunk and in later ones
    (freq_reduce overwrites on the first chunk and accumulates afterwards; the exact kernel adds into the same sums)"""
    gm, rc = handles
    with _knobs(switch, "8"):
        gm.run_dense(rc)
        launches = _ffi.last_call_stats(_ffi.PHMM_STATS_DENSE_FWD)[1]
        whole = _call(gm, rc)
        gpu_lib.phmm_set_workspace_limit(4 << 20)
        try:
            gm.run_dense(rc)
            launches_c = _ffi.last_call_stats(_ffi.PHMM_STATS_DENSE_FWD)[1]
            parts = _call(gm, rc)
        finally:
            gpu_lib.phmm_set_workspace_limit(0)
    print(f"switch {switch}: forward launches {launches} unlimited, {launches_c} under the limit")
    assert launches_c > launches
    for k in ("lf", "lb", "lf_e", "lf_o"):
        assert np.array_equal(np.isnan(whole[k]), np.isnan(parts[k])), k
        assert np.isnan(whole[k]).any() == switch
        assert np.allclose(whole[k], parts[k], atol=1e-12, rtol=0, equal_nan=True), k
    for k in ("nf", "ef", "inf"):
        assert np.allclose(whole[k], parts[k], atol=1e-10, rtol=0), k


def test_batch_of_flagged_reads_only(gpu_lib, family):
    fam = family
    deepest = np.argsort(fam.depth_both)[-5:]
    reads = [fam.reads[r] for r in deepest]
    gm, rc = D.PHMMModel(fam.arrays), D.ReadCollection(reads)
    with _knobs(True, None):
        assert np.isnan(gm.run_dense(rc)[0]).all()
    with _knobs(False, None):
        res = _call(gm, rc)
    for k, want in (("lf", fam.lf), ("lb", fam.lb), ("lf_e", fam.lf), ("lf_o", fam.lf)):
        assert np.all(np.isfinite(res[k])) and np.max(np.abs(res[k] - want[deepest])) <= TOL_EXACT, k
    for k, want in (("nf", fam.nf), ("ef", fam.ef), ("inf", fam.inf)):
        assert np.all(np.isfinite(res[k])) and np.max(np.abs(res[k] - want[deepest].sum(axis=0))) <= TOL_EXACT, k


@pytest.mark.parametrize("side", ["below", "above"])
def test_tables_either_side_of_the_flag(handles, family, switched, side):
    """phmm_dense_tables of the deepest chimera the certificate passes and of the shallowest it flags, at the junction
    column, its neighbours and both ends; the switch does not reach this entry point.

    The certificate of run_dense bounds the lost mass against P, not against a cell: with the scaled tables alone the
    backward tables of `below` (a = 196, depth 585 nats) held, at column 0, 126 cells per state that were finite and too
    small by up to 132 nats, the shallowest 250 nats below the column maximum, and reported cells 577 nats below it as
    -inf -- what is flushed behind the junction is missing from every cell before it whose best continuation ran
    through it.  phmm_dense_tables therefore certifies the cells as well (exact_dense.hip: certify_dense_cells) and
    returns the tables of the exact recursion for such a read.  See DESIGN.md section 3."""
    fam = family
    gm, _ = handles
    nan = np.isnan(switched["lf"])
    chim = fam.is_fwd
    if side == "below":
        r = int(np.flatnonzero(chim & ~nan)[np.argmax(fam.depth[chim & ~nan])])
    else:
        r = int(np.flatnonzero(chim & nan)[np.argmin(fam.depth[chim & nan])])
    read, a = fam.reads[r], int(fam.a[r])
    print(f"{side}: a = {a}, depth {fam.depth[r]:.1f} nats")
    with _knobs(True, None):
        out = gm.run(read)
    oo = fam.om.run(read)
    L = len(read)
    worst, shallowest, wrong = 0.0, (np.inf, None), []
    for i in (0, a - 1, a, a + 1, L - 1):
        for name, got, want in (("F", out.forward, oo.forward.table(i)), ("B", out.backward, oo.backward.table(i))):
            m, ins, d, sc = want
            top = max(m.max(), ins.max(), d.max())
            for t, g, w_ in (("m", got.m[i], m), ("i", got.i[i], ins), ("d", got.d[i], d)):
                # (the scaled domain flushes cells: the unflagged read's -inf cells are compared by their depth instead)
                lost = np.isneginf(g) & ~np.isneginf(w_) if side == "below" else np.zeros(g.size, bool)
                if lost.any() and float(np.min(top - w_[lost])) < shallowest[0]:
                    shallowest = (float(np.min(top - w_[lost])), (name, t, i))
                with np.errstate(invalid="ignore"):
                    worst = max(worst, float(np.max(np.abs(g - w_)[np.isfinite(g) & np.isfinite(w_)], initial=0.0)))
                off = ~(finite_close(g, w_, TOL_EXACT) | lost)
                if off.any():
                    wrong.append((name, t, i, int(off.sum()), float(np.min(top - w_[off]))))
        assert abs(out.forward.scal[i, 2] - oo.forward.table(i)[3][2]) <= TOL_EXACT
        assert abs(out.backward.scal[i, 0] - oo.backward.table(i)[3][0]) <= TOL_EXACT
    print(f"{side}: finite cells max |GPU - oracle| {worst:.3e}; shallowest cell reported -inf {shallowest[0]:.1f} nats "
          f"below its column maximum, at {shallowest[1]}; tables with finite cells off by more than {TOL_EXACT} "
          f"(table, state, column, cells, nats below the column maximum of the shallowest) {wrong}")
    assert not wrong, wrong
    assert shallowest[0] >= 700.0, shallowest
