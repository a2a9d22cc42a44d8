"""The oracle is indifferent to how nodes are numbered and edges are ordered (no GPU): every named ordering of
graph_cases.py on the DBG and on the zoo graph, oracle against relabelled oracle.  This proves the relabelled inputs
and the functions that carry lists, vectors and CSRs across a permutation before tests/test_gpu_relabel.py leans on
them, and that each ordering does to the chain fast path what its name says (chain_share).

Bounds: the oracle works in the log domain in float64; a relabelling changes the order in which the parents of a node
are log-added, a few ulps of values of magnitude <= ~1e3 (measured: 1.4e-14 on ln P, 2.8e-14 on node usage) -- 1e-12.
Mapping lists pass the plain compare_mappings: no tie retry is needed on the oracle side."""
import numpy as np
import pytest

import dbgphmm_amd as D
import graph_cases as G
from helpers import compare_mappings

TOL = 1e-12


def _dev(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)), initial=0.0))


@pytest.mark.parametrize("ordering", G.ORDERINGS)
@pytest.mark.parametrize("graph", G.GRAPHS)
def test_oracle_is_relabelling_invariant(oracle, graph, ordering):
    reads = G.base_case(graph)["reads"]
    c = G.relabelled_case(graph, ordering)
    npm, epm = c["node_perm"], c["edge_perm"]
    a, b = G.oracle_reference(graph), G.oracle_reference(graph, ordering)
    assert np.all(np.isfinite(a["lf"])) and np.all(np.isfinite(a["lp"]))
    dev = dict(lf=_dev(b["lf"], a["lf"]), lb=_dev(b["lb"], a["lb"]), nf=_dev(b["nf"][npm], a["nf"]),
               ef=_dev(b["ef"][epm], a["ef"]), inf=_dev(b["inf"][npm], a["inf"]), lp=_dev(b["lp"], a["lp"]),
               lp_hint=_dev(b["lp_hint"], a["lp_hint"]), mp_nf=_dev(b["mp_nf"][npm], a["mp_nf"]))
    print(graph, ordering, dev)
    assert max(dev.values()) < TOL, dev
    # the lists of the relabelled oracle, ids mapped back, are the lists of the as-built one
    back = G.carry_mappings(b["mp"], G.inverse(npm))
    compare_mappings(reads, back, a["mp"], ratio=c["arrays"].param.active_node_max_ratio)
    # carrying there and back is the identity
    there = G.carry_mappings(a["mp"], npm)
    assert np.array_equal(G.carry_mappings(there, G.inverse(npm))[1], a["mp"][1])


@pytest.mark.parametrize("graph", G.GRAPHS)
def test_orderings_do_what_their_names_say(graph):
    arrays = G.base_case(graph)["arrays"]
    share = {o: G.chain_share(G.relabelled_case(graph, o)["arrays"]) for o in G.ORDERINGS}
    share["as built"] = G.chain_share(arrays)
    print(graph, share)
    if graph != "dbg":
        # every weight of the zoo model carries the factor 0.97: no chain flag under any labelling
        assert max(share.values()) == 0.0
        return
    assert share["as built"] >= 0.8
    assert share["identity"] == share["as built"]  # the edge order alone does not touch it
    for o in ("random", "reverse", "interleave"):
        assert share[o] <= 0.05, (o, share[o])
    assert 0.3 < share["blocks"] < 0.9
    assert abs(share["shift3"] - share["as built"]) <= 4.0 / arrays.n_nodes  # the flags are kept up to the wrap


def test_zoo_graph_has_what_it_says():
    for arms, max_deg in ((7, 7), (0, 2), (9, 9)):
        sg = G.zoo_graph(arms=arms)
        n = sg.base.size
        assert n == 150 + 4 * arms
        pairs = list(zip(sg.edge_src.tolist(), sg.edge_dst.tolist()))
        assert (20, 20) in pairs and pairs.count((40, 41)) == 2 and (130, 100) in pairs
        assert sg.base[90] == D.graph.NULL_BASE and (89, 90) in pairs and (90, 91) in pairs
        deg = max(np.bincount(sg.edge_src, minlength=n).max(), np.bincount(sg.edge_dst, minlength=n).max())
        assert deg == max_deg
        arrays = G.zoo_model(sg)
        fin = np.isfinite(arrays.trans_logp)
        assert np.all(arrays.trans_logp[fin] < 0.0)
        rows = np.bincount(sg.edge_src[fin], weights=np.exp(arrays.trans_logp[fin]), minlength=n)
        assert np.all((rows == 0.0) | (np.abs(rows - 0.97) < 1e-12))


def test_carry_functions():
    """relabel and the carry functions on a hand-sized example, against explicit loops"""
    rng = np.random.default_rng(1)
    arrays = G.base_case("zoo")["arrays"]
    n, e = arrays.n_nodes, arrays.n_edges
    npm, epm = rng.permutation(n), rng.permutation(e)
    r = G.relabel(arrays, npm, epm)
    for v in range(0, n, 7):
        assert r.emission[npm[v]] == arrays.emission[v] and r.init_logp[npm[v]] == arrays.init_logp[v]
    for j in range(0, e, 5):
        assert r.edge_src[epm[j]] == npm[arrays.edge_src[j]] and r.edge_dst[epm[j]] == npm[arrays.edge_dst[j]]
        assert r.trans_logp[epm[j]] == arrays.trans_logp[j]
    assert r.param is arrays.param
    vec = rng.integers(0, 5, size=(3, n))
    assert all(G.carry_vector(vec, npm)[c, npm[v]] == vec[c, v] for c in range(3) for v in range(0, n, 11))
    off, node, cn = D.model.copy_num_changes(vec[0], vec[1:])
    off2, node2, cn2 = G.carry_changes((off, node, cn), npm)
    mat = np.repeat(G.carry_vector(vec[0], npm)[None, :], 2, axis=0)
    for c in range(2):
        mat[c, node2[int(off2[c]):int(off2[c + 1])]] = cn2[int(off2[c]):int(off2[c + 1])]
    assert np.array_equal(mat, G.carry_vector(vec[1:], npm))
    goff, gnodes = D.unitig_groups(G.base_case("zoo")["sg"])
    goff2, gnodes2 = G.carry_groups((goff, gnodes), npm)
    assert np.array_equal(goff2, goff) and np.array_equal(G.inverse(npm)[gnodes2], gnodes)
    # a node map from this graph into a graph of 2n nodes: v -> {2v, 2v+1} for even v, nothing for odd v
    mo = np.concatenate([[0], np.cumsum(np.where(np.arange(n) % 2 == 0, 2, 0))])
    mn = np.array([x for v in range(0, n, 2) for x in (2 * v, 2 * v + 1)])
    pto = rng.permutation(2 * n)
    mo2, mn2 = G.carry_node_map(mo, mn, npm, pto)
    for v in range(n):
        got = sorted(mn2[int(mo2[npm[v]]):int(mo2[npm[v] + 1])].tolist())
        assert got == sorted(pto[mn[int(mo[v]):int(mo[v + 1])]].tolist())
