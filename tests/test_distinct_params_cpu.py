"""CPU: the parameter set of tests/distinct_params.py, the oracle under it, and the power of the GPU test that uses it.

Every parameter set the suite ran before this file has p_MI = p_MD = p_ID = p_DI, p_II = p_DD, p_IM = p_DM,
p_random = ln 1/4 and p_match = ln(1 - p_mismatch) (item 1 records it).  tests/test_gpu_distinct_params.py holds every
kernel family to the oracle under a set without ties; this file shows that the oracle deserves it and that the bars of
the GPU file would see an exchanged pair:
  1. the set: fifteen different values, rows that sum to 1, the C struct round trip, and the ties of new() / uniform();
  2. the oracle's forward over lists is the sum over every path, enumerated from the model alone, on 24 tiny models
     whose fifteen parameters are all drawn at random (bar 1e-12), and the dense forward total when every node is listed;
  3. the oracle's dense backward tables equal a NumPy restatement of the reference's b_init / b_step, which names each
     of the nine transitions where the reference does (1e-12 of the column maximum, linear space).  Forward against
     backward is no check: the reference's backward total differs from its forward total under ANY parameters (its Del
     chain is cut at n_max_gaps on the other side), by 1e-3 per read here;
  4. power: each exchange of a tied pair, p_random put back to 1/4 and p_match put back to 1 - p_mismatch move every
     output of the oracle, on every read of both fixtures, by at least 100 times the bar the GPU test holds that output
     to;
  5. the fixtures are what distinct_params.py says they are."""
import math

import numpy as np
import pytest

import dbgphmm_amd as D
import distinct_params as P
from dbgphmm_amd.params import CPHMMParams
import large_k_cases as LK
from helpers import TIE_RULES, subset_csr
from test_gpu_list_tables import oracle_tables  # (the oracle helpers of the GPU files, as the GPU test uses them)
from test_gpu_states import oracle_states
from test_sample_paths_ref_cpu import N_TINY, enumerate_paths, tiny_int

NINF = -math.inf
LN_FLOOR = math.log(1e-12)
# the bars of tests/test_gpu_distinct_params.py per output, and the factor every change must clear
BARS = {"dense forward ln P": 1e-9, "dense backward ln P": 1e-9, "adaptive ln P": 1e-6, "hinted ln P": 1e-9,
        "node usage": 1e-7, "state posteriors": 1e-8, "forward list tables": 1e-8, "backward list tables": 1e-8,
        "edge frequencies": 1e-9}
FACTOR = 100.0


# ---------------------------------------------------------------- 1. the set itself
def test_fifteen_different_values_and_rows_that_sum_to_one():
    v = [P.LINEAR[k] for k in P.FIELDS]
    assert len(P.FIELDS) == 15 and len(set(v)) == 15 and len({round(math.log(x), 12) for x in v}) == 15
    L = P.LINEAR
    for row in (("p_MM", "p_MI", "p_MD"), ("p_IM", "p_II", "p_ID"), ("p_DM", "p_DI", "p_DD")):
        assert abs(sum(L[k] for k in row) + L["p_end"] - 1.0) < 1e-15, row
    p = P.params(24, gaps=6)
    assert p.n_warmup == 24 and p.n_max_gaps == 6 and all(getattr(p, k) == P.DISTINCT[k] for k in P.FIELDS)
    s = P.params(24, **P.swapped("p_MI", "p_MD"))
    assert s.p_MI == P.DISTINCT["p_MD"] and s.p_MD == P.DISTINCT["p_MI"] and s.p_ID == P.DISTINCT["p_ID"]
    assert len(P.changes()) == 6


def test_the_c_struct_round_trips_the_fifteen_doubles():
    p = P.params(24)
    c = p.to_c()
    names = [n for n, _ in CPHMMParams._fields_]
    assert set(P.FIELDS) == set(names[:15])
    for k in P.FIELDS:
        assert getattr(c, k) == getattr(p, k) == P.DISTINCT[k], k
    # field by field at the offsets of the header: fifteen doubles in declaration order, then the integer knobs
    raw = np.frombuffer(bytes(c), dtype=np.float64, count=15)
    assert raw.tolist() == [P.DISTINCT[n] for n in names[:15]]
    assert (c.n_active_nodes, c.n_warmup, c.n_max_gaps, c.warmup_threshold) == (40, 24, 4, 200)


def test_every_set_made_by_new_or_uniform_is_tied():
    """why this file exists"""
    sets = [D.PHMMParams.uniform(x) for x in (0.0, 0.001, 0.01, 0.05, 0.1)]
    sets += [D.PHMMParams.new(0.03, 0.02, 0.09, 2e-3, 40, 24), D.PHMMParams.new(0.01, 0.02, 0.3, 1e-5, 40, 12),
             D.PHMMParams.new(0.07, 0.11, 0.23, 0.01, 40, 16)]
    for p in sets:
        assert p.p_MI == p.p_MD == p.p_ID == p.p_DI == p.p_gap_open and p.p_II == p.p_DD == p.p_gap_ext
        assert p.p_IM == p.p_DM and p.p_random == math.log(0.25)
        assert p.p_match == (math.log(1.0 - math.exp(p.p_mismatch)) if p.p_mismatch > NINF else 0.0)
    import best_path_ref as B
    i = B.INT_LOGS
    assert i["p_MI"] == i["p_DI"] == i["p_MD"] == i["p_ID"] and i["p_II"] == i["p_DD"] and i["p_IM"] == i["p_DM"]


# ---------------------------------------------------------------- 2. the oracle's forward against enumeration
def _lse(values):
    v = [x for x in values if x > NINF]
    if not v:
        return NINF
    m = max(v)
    return m + math.log(sum(math.exp(x - m) for x in v))


def test_oracle_forward_is_the_sum_over_every_path(oracle):
    worst = worst_dense = 0.0
    finite = 0
    for seed in range(N_TINY):
        arrays, read, lists = tiny_int(seed % 3, seed)
        om = oracle.Model(arrays)
        with np.errstate(divide="ignore"):
            for ls, dense in ((lists, False), ([[0, 1, 2]] * 3, True)):
                want = _lse(v for _, v in enumerate_paths(arrays, read, ls).values())
                got = om.forward_score_only(read, oracle.Mapping.from_lists(ls))
                if want == NINF or got == NINF:
                    assert want == got, (seed, dense, want, got)
                    continue
                finite += 1
                worst = max(worst, abs(got - want))
                if dense:
                    worst_dense = max(worst_dense, abs(om.forward(read).full_prob() - want))
    print(f"{finite} finite cases of {2 * N_TINY}: oracle against enumeration at most {worst:.3e} over lists, "
          f"{worst_dense:.3e} for the dense forward (bar 1e-12)")
    assert finite >= N_TINY and worst <= 1e-12 and worst_dense <= 1e-12


# ---------------------------------------------------------------- 3. the oracle's backward against b_init / b_step
def backward_numpy(arrays, read):
    """backward.rs:197-211 (b_init) and 216-261, 299-555 (b_step: bd0, bdt, bm, bi, bib, bmb) over all nodes, in linear
    space -> (m[L, N], i[L, N], d[L, N], mb[L], ib[L]).  Each of the nine transitions stands where the reference has it."""
    p = arrays.param
    e = lambda x: math.exp(x) if x > NINF else 0.0  # noqa: E731
    MM, MI, MD, IM, II, ID, DM, DI, DD = (e(getattr(p, k)) for k in ("p_MM", "p_MI", "p_MD", "p_IM", "p_II", "p_ID",
                                                                  "p_DM", "p_DI", "p_DD"))
    match, mismatch, random, end = e(p.p_match), e(p.p_mismatch), e(p.p_random), e(p.p_end)
    N, L = arrays.n_nodes, len(read)
    src, dst = arrays.edge_src.astype(np.int64), arrays.edge_dst.astype(np.int64)
    with np.errstate(under="ignore"):
        t, init = np.exp(arrays.trans_logp), np.exp(arrays.init_logp)

    def over_childs(x):
        """sum over the childs l of k of t_kl x[l], for every k"""
        out = np.zeros(N)
        np.add.at(out, src, t * x[dst])
        return out

    m1, i1, ib1 = np.full(N, end), np.full(N, end), 0.0  # b_init: m, i, d = p_end; mb, ib, e = 0
    M, I, Dl, MB, IB = np.zeros((L, N)), np.zeros((L, N)), np.zeros((L, N)), np.zeros(L), np.zeros(L)
    for j in range(L - 1, -1, -1):
        emit = np.where(arrays.emission == read[j], match, mismatch)  # p_match_emit(l, emission)
        em1 = emit * m1
        # bd: bd0 = to match by p_DM, to ins by p_DI; then n_max_gaps times over the childs by p_DD
        bdt = DM * over_childs(em1) + DI * random * i1
        d0 = bdt.copy()
        for _ in range(int(p.n_max_gaps)):
            bdt = DD * over_childs(bdt)
            d0 += bdt
        # bm, bi: to match and del of the childs, to ins of the node itself
        M[j] = MM * over_childs(em1) + MD * over_childs(d0) + MI * random * i1
        I[j] = IM * over_childs(em1) + ID * over_childs(d0) + II * random * i1
        # bib, bmb: the same from Begin, over all nodes by init
        IB[j] = float(np.sum(init * (IM * em1 + ID * d0))) + II * random * ib1
        MB[j] = float(np.sum(init * (MM * em1 + MD * d0))) + MI * random * ib1
        Dl[j] = d0
        m1, i1, ib1 = M[j], I[j], IB[j]
    return M, I, Dl, MB, IB


def _backward_gap(oracle, arrays, read):
    """-> largest |oracle - restatement| over the tables of one read, linear, relative to the column maximum"""
    with np.errstate(divide="ignore"):
        T = oracle.Model(arrays).backward(read, oracle.BWD_DENSE)
    M, I, Dl, MB, IB = backward_numpy(arrays, read)
    worst = 0.0
    for j in range(len(read)):
        m, ins, d, s = T.table(j)
        with np.errstate(under="ignore"):
            got = np.concatenate([np.exp(m), np.exp(ins), np.exp(d), np.exp(s[:2])])
        want = np.concatenate([M[j], I[j], Dl[j], [MB[j], IB[j]]])
        top = want.max()
        if top == 0.0:
            assert got.max() == 0.0, j
            continue
        worst = max(worst, float(np.max(np.abs(got - want))) / top)
    return worst


def test_oracle_backward_tables_are_b_init_and_b_step(oracle):
    worst_tiny = max(_backward_gap(oracle, *tiny_int(seed % 3, seed)[:2]) for seed in range(N_TINY))
    f = P.dbg()
    worst_dbg = 0.0
    for gaps, r in zip((0, 4, 6), f["reads"][1:4]):
        worst_dbg = max(worst_dbg, _backward_gap(oracle, P.with_param(f["arrays"], P.params(24, gaps)), r[:20]))
    print(f"oracle backward against b_init / b_step: {worst_tiny:.3e} on {N_TINY} tiny models, {worst_dbg:.3e} on three reads "
          f"of dbg() cut to 20 bases at n_max_gaps 0, 4, 6 (bar 1e-12 of the column maximum)")
    assert worst_tiny <= 1e-12 and worst_dbg <= 1e-12


def test_forward_against_backward_is_not_a_check(oracle):
    """the reference's own recursion (backward.rs:367-551; its tests allow 0.01): the totals differ under tied
    parameters just as they do under DISTINCT"""
    f = P.dbg()
    for param in (D.PHMMParams.new(0.03, 0.02, 0.09, 2e-3, 40, 24), P.params(24)):
        lf, lb, _ = oracle.Model(P.with_param(f["arrays"], param)).run_dense_reads(f["reads"], n_threads=8)
        gap = np.abs(lf - lb)
        print(f"|forward - backward| per read: {gap.min():.2e} .. {gap.max():.2e}")
        assert gap.min() > 1e-4 and gap.max() < 0.1


# ---------------------------------------------------------------- 4. power
def _outputs(oracle, which, param):
    """every output the GPU test compares, per read, from the oracle under `param`, on the fixture's reads and on the
    lists the oracle generated under DISTINCT (the lists the GPU test hands to the list calls) -> {name: [per read]}"""
    f = P.dbg() if which == "dbg" else P.u20()
    arrays, reads = P.with_param(f["arrays"], param), f["reads"]
    om = oracle.Model(arrays)
    po, nd, _ = P.lists_of(which)
    lists = (po, nd, np.zeros(nd.size))
    off = P.offsets(reads)
    out = {}
    lf, lb, _ = om.run_dense_reads(reads, n_threads=8)
    out["dense forward ln P"], out["dense backward ln P"] = list(lf), list(lb)
    out["adaptive ln P"] = list(om.full_prob_reads(reads, None, True, n_threads=8))
    out["hinted ln P"] = list(om.full_prob_reads(reads, lists, True, n_threads=8))
    out["node usage"] = [om.generate_mappings([r], None, True, n_threads=1)[1] for r in reads]

    class _RC:
        offsets = off
    _, st = oracle_states(oracle, arrays, reads, _RC, (po, nd))
    tb = oracle_tables(oracle, arrays, reads, po, nd)
    e0 = [int(po[off[i]]) for i in range(len(reads) + 1)]
    out["state posteriors"] = [st[e0[i]:e0[i + 1]] for i in range(len(reads))]
    out["forward list tables"] = [tb["f"][e0[i]:e0[i + 1]] for i in range(len(reads))]
    out["backward list tables"] = [tb["b"][e0[i]:e0[i + 1]] for i in range(len(reads))]
    out["edge frequencies"] = []
    for i, r in enumerate(reads):
        o = om.run_with_mapping(r, oracle.Mapping(*subset_csr(off, lists, [i])))
        out["edge frequencies"].append(o.to_edge_and_init_freqs()[0])
    return out


def _moved(name, a, b):
    """how far one read's output moved: |d| of a score, the largest |d| of a vector; of log tables the largest |d| over
    the entries the GPU test holds at the bar (both values above ln 1e-12: posteriors as they are, table entries
    relative to the table's largest entry)"""
    a, b = np.asarray(a, float), np.asarray(b, float)
    if a.ndim == 0 or name in ("node usage", "edge frequencies"):
        return float(np.max(np.abs(a - b)))
    top = 0.0 if name == "state posteriors" else max(a.max(), b.max())
    hi = (a >= top + LN_FLOOR) & (b >= top + LN_FLOOR)
    return float(np.max(np.abs(a[hi] - b[hi])))


@pytest.fixture(scope="module")
def base_outputs(oracle):
    return {w: _outputs(oracle, w, P.params(24 if w == "dbg" else 40)) for w in ("dbg", "u20")}


@pytest.mark.parametrize("change", list(P.changes()))
def test_every_change_moves_every_output_by_100_bars(oracle, base_outputs, change):
    smallest, where = math.inf, None
    for which in ("dbg", "u20"):
        k = 24 if which == "dbg" else 40
        f = P.dbg() if which == "dbg" else P.u20()
        om = oracle.Model(f["arrays"])
        forced = [LK.switch_of(oracle, om, r)[1] > 400 for r in f["reads"]]
        got = _outputs(oracle, which, P.params(k, **P.changes()[change]))
        for name, bar in BARS.items():
            for i in range(len(f["reads"])):
                if name in ("adaptive ln P", "node usage") and forced[i]:
                    continue  # (dropped from the adaptive comparisons of the GPU test as well)
                factor = _moved(name, base_outputs[which][name][i], got[name][i]) / bar
                if factor < smallest:
                    smallest, where = factor, (which, name, i)
                assert factor >= FACTOR, (change, which, name, i, factor)
    print(f"{change}: the smallest move is {smallest:.3g} bars ({where[1]}, read {where[2]} of {where[0]}()); {FACTOR:.0f} are asked")


# ---------------------------------------------------------------- 5. the fixtures
def _tie_spread(oracle, om, reads):
    base = om.full_prob_reads(reads, None, True, n_threads=8)
    spread = 0.0
    for eps, mode in TIE_RULES:
        P.set_tie_rule(oracle, eps, mode)
        try:
            spread = max(spread, float(np.max(np.abs(om.full_prob_reads(reads, None, True, n_threads=8) - base))))
        finally:
            P.set_tie_rule(oracle, 0.0, 0)
    return base, spread


def test_fixture_dbg(oracle):
    f = P.dbg()
    arrays, reads = f["arrays"], f["reads"]
    assert arrays.n_nodes == 1118 and len(reads) == 8 and all(60 <= len(r) <= 120 for r in reads)
    om = oracle.Model(arrays)
    sw = [LK.switch_of(oracle, om, r) for r in reads]
    cols, forced = [s[0] for s in sw], [s[1] > 400 for s in sw]
    assert min(cols) >= 18 and max(cols) <= 24 and sum(forced) == 1 and sum(forced) <= len(reads) // 4
    adaptive, spread = _tie_spread(oracle, om, reads)
    lf, _, _ = om.run_dense_reads(reads, n_threads=8)
    print(f"dbg(): switch columns {cols}, forced {forced.index(True)}, |dense - adaptive| {np.max(np.abs(lf - adaptive)):.1e}, "
          f"tie spread {spread:.1e}")
    assert np.max(np.abs(lf - adaptive)) <= 3e-13 and spread <= 1e-12
    po, nd, _ = P.lists_of("dbg")
    assert int(np.diff(po.astype(np.int64)).max()) <= 64
    for width in P.PADS:
        ppo, pnd = P.padded("dbg", width)
        cnt = np.diff(ppo.astype(np.int64))
        assert int(cnt.max()) == width and ppo.size == po.size
        assert all(len(set(pnd[int(a):int(b)].tolist())) == b - a for a, b in zip(ppo[:64], ppo[1:65]))


def test_fixture_u20(oracle):
    f = P.u20()
    arrays, reads = f["arrays"], f["reads"]
    assert arrays.n_nodes == 555 and len(reads) == 6 and all(len(r) <= 200 for r in reads)
    assert all(getattr(arrays.param, k) == P.DISTINCT[k] for k in P.FIELDS) and arrays.param.n_warmup == 40
    om = oracle.Model(arrays)
    sw = [LK.switch_of(oracle, om, r) for r in reads]
    assert not any(s[1] > 400 for s in sw)  # no forced switch
    assert all(65 <= s[2] <= 400 for s in sw) and max(s[2] for s in sw) > 256  # the 400-slot / block classes
    _, spread = _tie_spread(oracle, om, reads)
    assert spread <= 1e-12
    po, _, _ = P.lists_of("u20")
    off = P.offsets(reads)
    cnt = np.diff(po.astype(np.int64))
    rmax = [int(cnt[off[i]:off[i + 1]].max()) for i in range(len(reads))]
    print(f"u20(): nodes at the switch {[s[1] for s in sw]}, first sparse columns {[s[2] for s in sw]}, longest lists {rmax}")
    assert all(65 <= m <= 400 for m in rmax)


def _largest_drop_bits(oracle, c):
    """the largest fall, in bits, of the top of the forward table (entries and InsBegin) from one base to the next of a
    cut read over its lists: the hinted kernels rescale by it and hand the read to the exact kernel below -512"""
    po, nd = c["lists"]
    mp = oracle.Mapping(po, nd, np.zeros(nd.size))
    with np.errstate(divide="ignore"):
        F = oracle.Model(c["arrays"]).forward(c["reads"][0], oracle.FWD_MAPPING, mp)
        tops = []
        for i in range(len(c["reads"][0])):
            m, ins, d, s = F.table(i)
            tops.append(max(m.max(), ins.max(), d.max(), s[1]))
    return float(np.diff(tops).min()) / math.log(2.0), F.full_prob()


def _certificate_nats(oracle, arrays, read):
    """what certify_dense (exact_dense.hip) bounds, from the oracle's tables: the largest ln max F[i] + ln max B[i + 1]
    - ln P; the scaled dense kernels are certified up to about (1022 - 64 - 50 - log2(6 N len)) ln 2 = 613 nats"""
    out = oracle.Model(arrays).run(read)
    top = lambda T, i: max(x.max() for x in T.table(i)[:3])  # noqa: E731
    lp = out.to_full_prob_forward()
    return max(top(out.forward, i) + min(max(top(out.backward, i + 1), top(out.backward, i)), 0.0) - lp for i in range(len(read) - 1))


def test_fixture_cut_reads_and_chimeras(oracle):
    """the cut read and the chimera of the fixtures stay on the scaled kernels; their deep forms reach the exact ones"""
    whole = oracle.Model(P.dbg()["arrays"])
    for c, at, deep in ((P.cut_read(), P.CUT_AT, False), (P.deep_cut_read(), P.DEEP_CUT_AT, True)):
        po, nd = c["lists"]
        r = c["reads"][0]
        assert po.size == len(r) + 1 and int(po[-1]) == nd.size
        victim = int(nd[int(po[at])])
        assert c["sg"].copy_num[victim] == 0 and P.dbg()["sg"].copy_num[victim] > 0
        bits, cut = _largest_drop_bits(oracle, c)
        uncut = whole.full_prob_reads([r], (po, nd, np.zeros(nd.size)), True, n_threads=1)[0]
        print(f"read of {len(r)} bases cut at {at}: ln P {cut:.3f} for {uncut:.3f} uncut, the largest fall of a column is {bits:.0f} bits")
        assert np.isfinite(cut) and cut < uncut - 100.0  # the InsBegin chain carries the bases before the cut
        assert bits < -700.0 if deep else -400.0 < bits < -150.0
    ch = P.chimera()
    assert len(ch) == 160 and ch[:60] == P.dbg()["reads"][0][:60] and ch[60:] == P.dbg()["reads"][1][:100]
    shallow = _certificate_nats(oracle, P.dbg()["arrays"], ch)
    arrays, deep_ch = P.deep_chimera()
    deep = _certificate_nats(oracle, arrays, deep_ch)
    print(f"chimera of {len(ch)} bases: {shallow:.0f} nats; deep chimera of {len(deep_ch)} bases on {arrays.n_nodes} nodes: {deep:.0f} nats "
          f"(the dense certificate holds to about 613, the scaled values are gone at 708)")
    assert shallow < 100.0 and deep > 750.0


def test_no_decision_of_a_walk_compared_word_for_word_is_near_a_boundary():
    """the condition tests/sample_paths_ref.py and tests/sample_reads_ref.py put on every fixture the GPU test compares
    word for word (the device's exp and Python's may differ in the last bits): every margin at least 1e-9.  A seed that
    fails gets replaced in distinct_params.py, never the threshold."""
    import best_path_ref as B
    import sample_paths_ref as S
    import sample_reads_ref as G
    for width in (None, 65, 400):
        arrays, reads, po, nd = P.walk_case(width)
        off = P.offsets(reads)
        assert int(np.diff(po.astype(np.int64)).max()) == (width or 49)
        lists = [B.lists_of(po, nd, off[j], off[j + 1]) for j in range(len(reads))]
        res = S.sample_set(arrays, reads, lists, 4, P.SAMPLE_SEED)
        m = min(r["margin"] for r in res)
        print(f"sampled paths, longest list {width or 49}: {len(reads)} reads x 4, the smallest margin is {m:.3e}")
        assert all(r["logz"] > NINF for r in res) and m >= S.MIN_MARGIN
    walks = [G.walk(P.dbg()["arrays"], P.GEN_SEED, w, P.GEN_LENGTH, G.STATE_COUNT, None) for w in range(P.GEN_WALKS)]
    m = min(w[3] for w in walks)
    print(f"generated reads: {len(walks)} walks of {P.GEN_LENGTH} states, the smallest margin is {m:.3e}")
    assert m >= 1e-9
