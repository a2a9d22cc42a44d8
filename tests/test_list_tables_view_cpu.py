"""CPU: the views of ListTables (dbgphmm_amd/model.py) held to the oracle.  A ListTables is built with from_arrays from
the oracle's own forward_with_mapping / backward_with_mapping tables on a small model, so nothing here needs a GPU: what
is tested is the index rule of table_merged (table.rs:414-434), the InsBegin posterior against to_emit_probs(p + 1)
(table.rs:500-505) and the order of top_states against a numpy restatement of to_states() (table.rs:228-238), exact
ties included.

The parameters are not uniform: under PHMMParams.uniform mb and ib of a backward table are equal and a swap of the two
would pass."""
import numpy as np
import pytest

import dbgphmm_amd as D
from helpers import subset_csr

PARAM = D.PHMMParams.new(0.01, 0.02, 0.3, 1e-5, 40, 12)


def oracle_tables(oracle, arrays, reads, po, nd):
    """forward(read, FWD_MAPPING, its lists) / backward(read, BWD_MAPPING, its lists) of every read, table(p) at the listed
    nodes -> dict of the six arrays of phmm_run_with_mapping_tables"""
    om = oracle.Model(arrays)
    off = np.zeros(len(reads) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
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


@pytest.fixture(scope="module")
def case(oracle):
    hap = D.random_genome(300, 7)
    sg = D.dbg_from_haplotypes([hap, D.diverge(hap, 0.02, 8)], 12)
    arrays = D.vectorised_to_phmm(sg, PARAM, 0)
    reads = D.sample_reads(arrays, 10 ** 9, 60, seed=3, max_reads=3)
    reads = [reads[0], reads[1][:1], reads[2][:2]]
    (po, nd, _), _ = oracle.Model(arrays).generate_mappings(reads, None, True, n_threads=2)
    t = oracle_tables(oracle, arrays, reads, po, nd)
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads])
    lt = D.ListTables.from_arrays(off, po, nd, arrays.param.p_end, arrays.n_nodes, t["f"], t["fs"], t["b"], t["bs"])
    return arrays, reads, (po.astype(np.int64), nd), t, lt


def _outputs(oracle, arrays, reads, po, nd):
    om = oracle.Model(arrays)
    off = np.zeros(len(reads) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    for i, r in enumerate(reads):
        mp = oracle.Mapping(*subset_csr(off, (po.astype(np.uint64), nd, np.zeros(nd.size)), [i]))
        with np.errstate(divide="ignore"):
            yield i, r, om.run_with_mapping(r, mp)


def test_totals_come_from_the_scalars(case):
    arrays, reads, (po, nd), t, lt = case
    assert len(lt) == 3 and [lt.read_len(r) for r in range(3)] == [len(r) for r in reads]
    assert np.array_equal(lt.logp_forward, t["lf"]) and np.array_equal(lt.logp_backward, t["lb"])
    # (the two totals need not be equal: the forward and the backward pass lose different paths to the lists)
    assert np.all(np.isfinite(t["lf"])) and np.max(np.abs(t["lf"] - t["lb"])) < 0.1
    for r in range(3):
        assert lt.prefix_logp(r)[-1] == lt.logp_forward[r] and lt.suffix_logp(r)[0] == lt.logp_backward[r]
    # mb and ib of a backward table differ under these parameters, by a quarter of a nat at the median: a swap cannot hide
    assert np.median(np.abs(t["bs"][:, 0] - t["bs"][:, 1])) > 0.2 and np.all(t["bs"][:, 0] != t["bs"][:, 1])


def test_table_merged_follows_the_reference_index_rule(oracle, case):
    arrays, reads, (po, nd), t, lt = case
    for i, r, out in _outputs(oracle, arrays, reads, po, nd):
        L = len(r)
        for kind, T in (("forward", out.forward), ("backward", out.backward)):
            for idx in sorted({0, L - 1, L}):
                # the oracle's table by the rule of table.rs:414-434; -1 is its init table
                ti = (-1 if idx == 0 else idx - 1) if kind == "forward" else (-1 if idx >= L else idx)
                m, ins, d, s = T.table(ti)
                nodes, vals, scal = lt.table_merged(kind, i, idx)
                want = np.stack([m[nodes], ins[nodes], d[nodes]], axis=1)
                assert np.array_equal(vals, want), (kind, i, idx)
                assert np.array_equal(scal, s), (kind, i, idx, scal, s)
                # and no mass outside the nodes the view names
                rest = np.ones(arrays.n_nodes, dtype=bool)
                rest[nodes] = False
                assert np.all(m[rest] == -np.inf) and np.all(ins[rest] == -np.inf) and np.all(d[rest] == -np.inf)
    with pytest.raises(ValueError):
        lt.table_merged("sideways", 0, 0)
    with pytest.raises(IndexError):
        lt.forward(0, len(reads[0]))


def test_ins_begin_posterior_is_the_ib_scalar_of_to_emit_probs(oracle, case):
    arrays, reads, (po, nd), t, lt = case
    worst = 0.0
    for i, r, out in _outputs(oracle, arrays, reads, po, nd):
        got = lt.ins_begin_posterior(i)
        assert got.shape == (len(r),) and got[-1] == -np.inf  # b_init.ib = 0
        for p in range(len(r)):
            want = out.to_emit_probs(p + 1)[3][1]
            if want == -np.inf or got[p] == -np.inf:
                assert want == got[p], (i, p, want, got[p])
            else:
                worst = max(worst, abs(want - got[p]))
    print(f"InsBegin posterior: max |d| {worst:.3e}")
    assert worst < 1e-9


def _numpy_states(nodes, vals, n):
    """Match.. Ins.. Del.. in slot order, stable ascending sort, reversed, head n (table.rs:228-238)"""
    k = nodes.shape[0]
    rows = [(int(nodes[j]), kind, float(vals[j, c])) for c, kind in enumerate("MID") for j in range(k)]
    order = sorted(range(len(rows)), key=lambda a: rows[a][2])  # (sorted is stable)
    return [rows[a] for a in order[::-1][:n]]


def test_top_states_order(case):
    arrays, reads, (po, nd), t, lt = case
    for kind in ("forward", "backward"):
        for pos in (0, 5, len(reads[0]) - 1):
            nodes, vals, _ = lt.forward(0, pos) if kind == "forward" else lt.backward(0, pos)
            for n in (1, 3, 3 * nodes.shape[0], 3 * nodes.shape[0] + 5):
                got = lt.top_states(kind, 0, pos, n)
                assert got == _numpy_states(nodes, vals, n), (kind, pos, n)
                assert len(got) == min(n, 3 * nodes.shape[0])
    assert lt.top_states("forward", 0, 0, 0) == []


def test_top_states_exact_ties():
    """three entries whose values tie across kinds and slots: Del before Ins before Match, the later slot first"""
    nodes = np.array([7, 3, 9], dtype=np.uint32)
    f = np.array([[-1.0, -1.0, -2.0], [-1.0, -np.inf, -1.0], [-3.0, -1.0, -1.0]])
    lt = D.ListTables.from_arrays([0, 1], [0, 3], nodes, -11.5, 10, forward=f, forward_scalars=np.array([[-4.0, -5.0]]))
    got = lt.top_states("forward", 0, 0, 9)
    assert got == _numpy_states(nodes, f, 9)
    assert got[:6] == [(9, "D", -1.0), (3, "D", -1.0), (9, "I", -1.0), (7, "I", -1.0), (3, "M", -1.0), (7, "M", -1.0)]
    assert got[-1] == (3, "I", -np.inf)
    assert lt.bwd is None and lt.logp_backward is None and lt.logp_forward[0] == -5.0
    assert np.array_equal(lt.table_merged("backward", 0, 1)[1], np.full((10, 3), -11.5))
