"""No GPU: link_keys (the edge map "ordered pair of node groups -> key" of run_with_mapping_read_edges) on the toy graphs of
tests/golden/toy_dbgs.json and on a hand-built bubble, and the views of ReadEdges on rows built from plain arrays."""
import json
import math
import os

import numpy as np
import pytest

import dbgphmm_amd as D
from dbgphmm_amd import formats as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_KEY = D.PHMM_NO_KEY


def _check_link_keys(src, dst, groups, edge_key, links):
    """the definition, edge by edge"""
    g_off, g_nodes = np.asarray(groups[0], dtype=np.int64), np.asarray(groups[1], dtype=np.int64)
    g_of = {}
    for g in range(g_off.size - 1):
        for v in g_nodes[g_off[g]:g_off[g + 1]].tolist():
            g_of[v] = g
    assert edge_key.dtype == np.uint32 and edge_key.shape == (len(src),)
    assert links.shape[1] == 2 and len({tuple(p) for p in links.tolist()}) == links.shape[0]  # equal pairs share a key
    assert links.tolist() == sorted(links.tolist())
    used = set()
    for e, (a, b) in enumerate(zip(src.tolist(), dst.tolist())):
        ga, gb = g_of.get(a), g_of.get(b)
        if ga is None or gb is None or ga == gb:  # an end in no group, or inside one group
            assert edge_key[e] == NO_KEY, e
        else:
            assert edge_key[e] < links.shape[0] and tuple(links[edge_key[e]]) == (ga, gb), e
            used.add(int(edge_key[e]))
    assert used == set(range(links.shape[0]))  # no key without an edge


@pytest.mark.parametrize("name", ["circular", "linear", "intersection", "selfloop", "repeat"])
def test_link_keys_on_the_toy_graphs(name):
    toy = json.load(open(os.path.join(ROOT, "tests", "golden", "toy_dbgs.json")))[name]
    sg = F.dbg_from_seq_graph_kmers([x.encode() for x in toy["kmers"]], toy["copy_nums"], toy["k"]).to_seq_graph()
    arrays = D.vectorised_to_phmm(sg, D.PHMMParams.default(), 1)
    groups = D.unitig_groups(sg)
    edge_key, links = D.link_keys(arrays, groups)
    _check_link_keys(arrays.edge_src, arrays.edge_dst, groups, edge_key, links)
    # unitigs cover every node: an edge is inside a unitig or a link
    G = groups[0].size - 1
    if G > 1:
        assert links.shape[0] > 0
    # with every other group dropped, the edges at its nodes lose their keys
    keep = list(range(0, G, 2))
    off, nodes = [0], []
    for g in keep:
        nodes.extend(groups[1][int(groups[0][g]):int(groups[0][g + 1])].tolist())
        off.append(len(nodes))
    part = (np.array(off, dtype=np.uint64), np.array(nodes, dtype=np.uint32))
    ek2, links2 = D.link_keys(sg, part)  # (a SeqGraph serves as well)
    _check_link_keys(sg.edge_src, sg.edge_dst, part, ek2, links2)


def test_link_keys_on_a_hand_built_bubble():
    """0 -> 1 -> {2 -> 3, 4 -> 5} -> 6 -> 7, a second parallel edge 1 -> 2 and an ungrouped node 8 behind 7:
    groups A = {0, 1}, B = {2, 3}, C = {4, 5}, D = {6, 7}"""
    class G:
        edge_src = np.array([0, 1, 1, 2, 4, 3, 5, 6, 7, 1, 8], dtype=np.uint32)
        edge_dst = np.array([1, 2, 4, 3, 5, 6, 6, 7, 8, 2, 0], dtype=np.uint32)
    groups = (np.array([0, 2, 4, 6, 8], dtype=np.uint64), np.array([0, 1, 2, 3, 4, 5, 6, 7], dtype=np.uint32))
    edge_key, links = D.link_keys(G, groups)
    assert links.tolist() == [[0, 1], [0, 2], [1, 3], [2, 3]]
    #                            0->1    1->2 1->4 2->3    4->5    3->6 5->6 6->7    7->8    1->2 8->0
    assert edge_key.tolist() == [NO_KEY, 0, 1, NO_KEY, NO_KEY, 2, 3, NO_KEY, NO_KEY, 0, NO_KEY]
    _check_link_keys(G.edge_src, G.edge_dst, groups, edge_key, links)
    # no groups at all, and one group of everything: nothing is keyed
    for gr in ((np.array([0], dtype=np.uint64), np.zeros(0, dtype=np.uint32)),
               (np.array([0, 9], dtype=np.uint64), np.arange(9, dtype=np.uint32))):
        ek, ln = D.link_keys(G, gr)
        assert np.all(ek == NO_KEY) and ln.shape == (0, 2)


def test_read_edges_from_plain_arrays():
    """3 reads over E = 4 edges and N = 3 nodes under the default keys (K = 7)"""
    E, N = 4, 3
    row_off, keys = [0, 3, 3, 6], [1, 3, 5, 0, 1, 4]
    usage = [.5, .25, 1., .125, 2., .75]
    totals = np.array([.125, 2.5, 0., .25, .75, 1., 0.])
    end_terms = np.array([[1e-3, 2e-3], [0., 0.], [4e-3, 8e-3]])
    u = D.ReadEdges.from_arrays(E + N, row_off, keys, usage, totals=totals, end_terms=end_terms, n_edges=E)
    assert len(u) == 3 and u.n_keys == 7 and u.n_edges == E
    a = u.arrays()
    assert a[0].dtype == np.uint64 and a[1].dtype == np.uint32 and a[2].shape == (6,) and u.export()[2] is a[2]
    assert u.row(0)[0].tolist() == [1, 3, 5] and u.row(0)[1].tolist() == [.5, .25, 1.]
    assert u.row(1)[0].size == 0 and u.row(1)[1].size == 0
    assert u.edge_freqs(0).tolist() == [0., .5, 0., .25] and u.edge_freqs(1).tolist() == [0.] * 4
    assert u.edge_freqs(2).tolist() == [.125, 2., 0., 0.]
    # reads_of is the transpose of row
    for key in range(7):
        rd, us = u.reads_of(key)
        want = [(r, float(u.row(r)[1][u.row(r)[0].tolist().index(key)])) for r in range(3) if key in u.row(r)[0].tolist()]
        assert list(zip(rd.tolist(), us.tolist())) == want, key
    assert u.reads_of(1)[0].tolist() == [0, 2] and u.reads_of(2)[0].size == 0
    # the totals are the column sums of the rows
    cols = np.zeros(7)
    np.add.at(cols, np.array(keys), np.array(usage))
    assert np.array_equal(cols, u.totals)

    # init_freqs: the row value at key E + v plus init_v (A_r + T_r e_v(last base))
    class Arr:
        param = D.PHMMParams.default()
        init_logp = np.log(np.array([.5, .25, .25]))
        emission = np.frombuffer(b"ACA", dtype=np.uint8)
    pm, px = math.exp(Arr.param.p_match), math.exp(Arr.param.p_mismatch)
    init = np.exp(Arr.init_logp)
    got = u.init_freqs(0, Arr, ord("A"))
    want = np.array([0., 1., 0.]) + init * (1e-3 + 2e-3 * np.array([pm, px, pm]))
    assert np.array_equal(got, want)
    got = u.init_freqs(2, Arr, ord("C"))
    want = np.array([.75, 0., 0.]) + init * (4e-3 + 8e-3 * np.array([px, pm, px]))
    assert np.array_equal(got, want)
    assert np.array_equal(u.init_freqs(1, Arr, ord("G")), np.zeros(3))
    # under a caller's map the dense views by edge are refused
    v = D.ReadEdges.from_arrays(2, [0, 1], [1], [.5])
    assert v.key_freqs(0).tolist() == [0., .5]
    with pytest.raises(ValueError):
        v.edge_freqs(0)
    with pytest.raises(ValueError):
        v.init_freqs(0, Arr, ord("A"))
