"""The definition behind phmm_run_with_mapping_read_usage, on the CPU: the numpy restatement (read_usage_ref.py) fed the
oracle's to_emit_probs(p + 1) at the listed nodes gives, per read and node, M + I + D = the oracle's
run_with_mapping(read, lists).to_node_freqs() -- so the values of the states call define the rows.  Bar 1e-13: each sum
has at most 9 terms of at most 1 (2.2e-16 was measured).  Then the restatement's own structure: keys, groups, dropped
nodes, empty groups and lists, a one-base read, duplicates.  No GPU needed."""
import numpy as np
import pytest

import dbgphmm_amd as D
from helpers import small_dbg_model, subset_csr
from read_usage_ref import NONE, key_map, read_usage_ref

N_READS = 12


@pytest.fixture(scope="module")
def probe(oracle):
    """the first 12 reads of the 70-read fixture, the oracle's own lists, its emit probs at the listed nodes"""
    arrays, _ = small_dbg_model(300, 12, 0.01, seed=5)
    reads = D.sample_reads(arrays, 10 ** 9, 60, seed=70, max_reads=70)
    reads = [r[: max(1, len(r) - (j * 7) % 31)] for j, r in enumerate(reads)][:N_READS]
    om = oracle.Model(arrays)
    (po, nd, lp), _ = om.generate_mappings(reads, None, True, n_threads=4)
    off = np.zeros(len(reads) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    po = po.astype(np.int64)
    sl = np.full((int(po[-1]), 3), np.nan)
    freqs = []
    with np.errstate(divide="ignore"):
        for i, r in enumerate(reads):
            o = om.run_with_mapping(r, oracle.Mapping(*subset_csr(off, (po.astype(np.uint64), nd, lp), [i])))
            freqs.append(o.to_node_freqs())
            for p in range(len(r)):
                a0, a1 = int(po[off[i] + p]), int(po[off[i] + p + 1])
                m, ins, d, _ = o.to_emit_probs(p + 1)
                v = nd[a0:a1]
                sl[a0:a1, 0], sl[a0:a1, 1], sl[a0:a1, 2] = m[v], ins[v], d[v]
    assert not np.any(np.isnan(sl))
    return arrays.n_nodes, off, po, nd, sl, np.array(freqs)


def test_rows_are_the_oracles_node_freqs(probe):
    n_nodes, off, po, nd, sl, freqs = probe
    row_off, keys, usage, totals, terms = read_usage_ref(off, po, nd, sl, n_nodes)
    assert row_off.shape == (N_READS + 1,) and int(row_off[-1]) == keys.size == usage.shape[0]
    assert terms.max() <= 9
    worst = 0.0
    for r in range(N_READS):
        e0, e1 = int(row_off[r]), int(row_off[r + 1])
        dense = np.zeros(n_nodes)
        dense[keys[e0:e1]] = usage[e0:e1, 0] + usage[e0:e1, 1] + usage[e0:e1, 2]
        worst = max(worst, float(np.max(np.abs(dense - freqs[r]))))
        # keys are np.unique of the read's entries
        assert np.array_equal(keys[e0:e1], np.unique(nd[int(po[off[r]]):int(po[off[r + 1]])]))
    print(f"max |M + I + D - to_node_freqs| over {N_READS} reads: {worst:.3e} (bound 1e-13)")
    assert worst <= 1e-13
    # the totals are the rows summed over the reads
    dense = np.zeros((n_nodes, 3))
    np.add.at(dense, keys, usage)
    assert np.max(np.abs(dense - totals)) <= 1e-13
    assert np.max(np.abs(totals.sum(axis=1) - freqs.sum(axis=0))) <= 1e-12


def test_groups(probe):
    n_nodes, off, po, nd, sl, _ = probe
    node_form = read_usage_ref(off, po, nd, sl, n_nodes)
    # singleton groups in node order are the node form
    ident = (np.arange(n_nodes + 1, dtype=np.uint64), np.arange(n_nodes, dtype=np.uint32))
    single = read_usage_ref(off, po, nd, sl, n_nodes, ident)
    assert all(np.array_equal(a, b) for a, b in zip(node_form, single))
    # node % 3: the node rows summed by group
    order = np.argsort(np.arange(n_nodes) % 3, kind="stable").astype(np.uint32)
    cnt = np.bincount(np.arange(n_nodes) % 3, minlength=3)
    mod3 = (np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64), order)
    row_off, keys, usage, totals, terms = read_usage_ref(off, po, nd, sl, n_nodes, mod3)
    assert totals.shape == (3, 3)
    for r in range(N_READS):
        e0, e1 = int(node_form[0][r]), int(node_form[0][r + 1])
        want = np.zeros((3, 3))
        np.add.at(want, node_form[1][e0:e1] % 3, node_form[2][e0:e1])
        g0, g1 = int(row_off[r]), int(row_off[r + 1])
        assert np.array_equal(keys[g0:g1], np.unique(node_form[1][e0:e1] % 3))
        assert np.max(np.abs(usage[g0:g1] - want[keys[g0:g1]])) <= 1e-13
        assert int(terms[g0:g1].sum()) == int(po[off[r + 1]] - po[off[r]])
    # odd nodes in no group, an empty group in the middle: group 0 = nodes 0 mod 4, group 1 empty, group 2 = nodes 2 mod 4
    even = np.arange(0, n_nodes, 2, dtype=np.uint32)
    g0_nodes, g2_nodes = even[even % 4 == 0], even[even % 4 == 2]
    part = (np.array([0, g0_nodes.size, g0_nodes.size, g0_nodes.size + g2_nodes.size], dtype=np.uint64),
            np.concatenate([g0_nodes, g2_nodes]))
    key_of, K = key_map(n_nodes, part)
    assert K == 3 and np.all(key_of[1::2] == NONE)
    row_off, keys, usage, totals, terms = read_usage_ref(off, po, nd, sl, n_nodes, part)
    assert set(keys.tolist()) <= {0, 2} and np.all(totals[1] == 0.0)
    kept = int(np.sum(nd % 2 == 0))
    assert int(terms.sum()) == kept < nd.size


def test_edge_shapes():
    # an empty read set, a read without bases, a one-base read, empty lists, a node twice in a list
    row_off, keys, usage, totals, terms = read_usage_ref([0], [0], [], np.zeros((0, 3)), 4)
    assert row_off.tolist() == [0] and keys.size == 0 and usage.shape == (0, 3) and np.all(totals == 0) and totals.shape == (4, 3)
    read_off = [0, 0, 1, 4]                  # read 0 empty, read 1 one base, read 2 three bases
    pos_off = [0, 2, 2, 5, 6]                # base 1 (the first of read 2) has an empty list
    nodes = [3, 1, 2, 2, 0, 3]               # node 2 twice at one position
    with np.errstate(divide="ignore"):       # (log(0) = -inf)
        sl = np.log(np.array([[.5, .25, 0.], [.125, 0., .0625], [.25, .125, .0625], [.5, .0625, .03125], [0., 0., 0.],
                              [.125, .25, .5]]))
    row_off, keys, usage, totals, terms = read_usage_ref(read_off, pos_off, nodes, sl, 4)
    assert row_off.tolist() == [0, 0, 2, 5]
    assert keys.tolist() == [1, 3, 0, 2, 3] and terms.tolist() == [1, 1, 1, 2, 1]
    want = np.array([[.125, 0., .0625], [.5, .25, 0.], [0., 0., 0.], [.75, .1875, .09375], [.125, .25, .5]])
    assert np.allclose(usage, want, rtol=1e-14, atol=0.0) and np.array_equal(usage == 0.0, want == 0.0)
    assert np.allclose(totals, [[0., 0., 0.], [.125, 0., .0625], [.75, .1875, .09375], [.625, .5, .5]], rtol=1e-14, atol=0.0)
