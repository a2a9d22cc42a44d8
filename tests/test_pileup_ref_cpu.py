"""The definition behind phmm_run_with_mapping_pileup, on the CPU: the numpy restatement (pileup_ref.py) is held to a
direct triple loop over the header's definition on random small CSRs (empty lists, duplicates, a read of one base, -inf
values); the Pileup views and the pileup file are checked on its results; and one semantic case runs on the oracle's
dense run: six reads over a substituted base make exactly one node disagree with its emission.  No GPU needed."""
import io
import math

import numpy as np
import pytest

import dbgphmm_amd as D
from dbgphmm_amd import formats
from pileup_ref import CODE, entry_positions, pileup_ref
from read_usage_ref import read_usage_ref


def random_csr(rng, n_nodes, read_lens):
    """reads of the given lengths (0 allowed here: the restatement takes it), lists of 0..5 nodes with duplicates, about
    a fifth of the values -inf"""
    read_off = np.concatenate([[0], np.cumsum(read_lens)]).astype(np.int64)
    P = int(read_off[-1])
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=P)]
    widths = rng.integers(0, 6, size=P)
    if P:
        widths[0] = 0  # an empty list at the first position ...
        widths[-1] = 0  # ... and at the last
    pos_off = np.concatenate([[0], np.cumsum(widths)]).astype(np.int64)
    nodes = rng.integers(0, n_nodes, size=int(pos_off[-1]))
    with np.errstate(divide="ignore"):
        sl = np.log(rng.random((nodes.size, 3)) * (rng.random((nodes.size, 3)) > 0.2))
    return read_off, bases, pos_off, nodes, sl


def direct(read_off, bases, pos_off, nodes, sl, n_nodes):
    """the definition, entry by entry: read r, position p, place in the list -> {(r, key): [M, I, D] terms}"""
    seg = {}
    with np.errstate(under="ignore"):
        prob = np.exp(np.asarray(sl, dtype=np.float64).reshape(-1, 3))  # (the restatement's exp: the grouping is on trial)
    for r in range(len(read_off) - 1):
        for g in range(int(read_off[r]), int(read_off[r + 1])):
            for a in range(int(pos_off[g]), int(pos_off[g + 1])):
                key = 4 * int(nodes[a]) + "ACGT".index(chr(bases[g]))
                seg.setdefault((r, key), []).append(prob[a].tolist())
    return seg


@pytest.mark.parametrize("seed", range(6))
def test_restatement_is_the_definition(seed):
    rng = np.random.default_rng(seed)
    n_nodes = int(rng.integers(1, 7))
    lens = [1] + rng.integers(0, 9, size=int(rng.integers(1, 6))).tolist() + [1]
    read_off, bases, pos_off, nodes, sl = random_csr(rng, n_nodes, lens)
    row_off, keys, usage, totals, terms = pileup_ref(read_off, bases, pos_off, nodes, sl, n_nodes)
    seg = direct(read_off, bases, pos_off, nodes, sl, n_nodes)
    R = len(lens)
    assert row_off.shape == (R + 1,) and int(row_off[-1]) == keys.size == usage.shape[0] == terms.size == len(seg)
    want_tot = [[[] for _ in range(9)] for _ in range(n_nodes)]
    for r in range(R):
        e0, e1 = int(row_off[r]), int(row_off[r + 1])
        assert keys[e0:e1].tolist() == sorted(k for (rr, k) in seg if rr == r)
        for e in range(e0, e1):
            t = seg[(r, int(keys[e]))]
            assert terms[e] == len(t)
            for s in range(3):
                assert usage[e, s] == math.fsum(x[s] for x in t)
            v, c = divmod(int(keys[e]), 4)
            want_tot[v][c].append(usage[e, 0])
            want_tot[v][4 + c].append(usage[e, 1])
            want_tot[v][8].append(usage[e, 2])
    assert int(terms.sum()) == nodes.size
    assert np.array_equal(totals, np.array([[math.fsum(c) for c in node] for node in want_tot]).reshape(n_nodes, 9))
    # summed over the bases the rows are those of the read-usage restatement
    u_off, u_keys, u_usage, u_tot, _ = read_usage_ref(read_off, pos_off, nodes, sl, n_nodes)
    for r in range(R):
        assert np.array_equal(np.unique(keys[int(row_off[r]):int(row_off[r + 1])] >> 2), u_keys[int(u_off[r]):int(u_off[r + 1])])
    assert np.allclose(totals[:, 0:4].sum(axis=1), u_tot[:, 0], rtol=1e-13, atol=0.0)
    assert np.allclose(totals[:, 4:8].sum(axis=1), u_tot[:, 1], rtol=1e-13, atol=0.0)
    assert np.allclose(totals[:, 8], u_tot[:, 2], rtol=1e-13, atol=0.0)


def test_edge_shapes():
    # no reads; then: read 0 one base, read 1 three bases whose first and last lists are empty, node 2 twice at a position
    row_off, keys, usage, totals, terms = pileup_ref([0], b"", [0], [], np.zeros((0, 3)), 3)
    assert row_off.tolist() == [0] and keys.size == 0 and usage.shape == (0, 3) and totals.shape == (3, 9) and np.all(totals == 0)
    read_off, bases = [0, 1, 4], b"TACG"
    pos_off = [0, 2, 2, 5, 5]
    nodes = [2, 0, 1, 2, 2]
    assert entry_positions(pos_off, 0, 5).tolist() == [0, 0, 2, 2, 2]  # the empty lists at 1 and 3 are passed over
    with np.errstate(divide="ignore"):
        sl = np.log(np.array([[.5, .25, 0.], [.125, 0., .0625], [0., 0., 0.], [.25, .125, .0625], [.5, .0625, .03125]]))
    row_off, keys, usage, totals, terms = pileup_ref(read_off, bases, pos_off, nodes, sl, 3)
    assert row_off.tolist() == [0, 2, 4]
    assert keys.tolist() == [4 * 0 + 3, 4 * 2 + 3, 4 * 1 + 1, 4 * 2 + 1] and terms.tolist() == [1, 1, 1, 2]
    want = np.array([[.125, 0., .0625], [.5, .25, 0.], [0., 0., 0.], [.75, .1875, .09375]])
    assert np.allclose(usage, want, rtol=1e-14, atol=0.0) and np.array_equal(usage == 0.0, want == 0.0)
    assert np.allclose(totals[2], [0., .75, 0., .5, 0., .1875, 0., .25, .09375], rtol=1e-14, atol=0.0)
    assert np.all(totals[1] == 0.0)  # the key stays in the row, with zeros
    with pytest.raises(AssertionError):
        pileup_ref(read_off, b"TANG", pos_off, nodes, sl, 3)


def test_pileup_views_and_file():
    """Fails without the feature: D.Pileup and formats.write_pileup do not exist."""
    rng = np.random.default_rng(11)
    n_nodes = 6
    read_off, bases, pos_off, nodes, sl = random_csr(rng, n_nodes, [1, 7, 4, 8, 1])
    row_off, keys, usage, totals, _ = pileup_ref(read_off, bases, pos_off, nodes, sl, n_nodes)
    pu = D.Pileup.from_arrays(n_nodes, row_off, keys, usage, totals)
    assert len(pu) == 5 and pu.n_nodes == n_nodes and pu.totals.shape == (n_nodes, 9)
    assert all(np.array_equal(a, b) for a, b in zip(pu.arrays(), (row_off, keys, usage)))
    for r in range(5):
        nd, bc, us = pu.row(r)
        e0, e1 = int(row_off[r]), int(row_off[r + 1])
        assert np.array_equal(4 * nd + bc, keys[e0:e1]) and np.array_equal(us, usage[e0:e1]) and np.all(bc < 4)
    for v in range(n_nodes):
        for c in range(4):
            rd, us = pu.reads_of(v, c)
            want = [r for r in range(5) if 4 * v + c in keys[int(row_off[r]):int(row_off[r + 1])].tolist()]
            assert rd.tolist() == want
            for r, x in zip(rd.tolist(), us):
                nd, bc, ru = pu.row(r)
                assert np.array_equal(ru[np.searchsorted(4 * nd + bc, 4 * v + c)], x)
    assert np.array_equal(pu.match_counts, totals[:, :4]) and np.array_equal(pu.ins_counts, totals[:, 4:8])
    assert np.array_equal(pu.del_counts, totals[:, 8]) and np.array_equal(pu.depth(), totals[:, :4].sum(axis=1))
    # without the totals of a call they are the rows summed on the host
    own = D.Pileup.from_arrays(n_nodes, row_off, keys, usage).totals
    assert np.allclose(own, totals, rtol=1e-13, atol=0.0)
    # hand-made totals: consensus, disagreements, the error profile
    t = np.zeros((4, 9))
    t[0, :4] = [5., 0., 1., 0.]      # emits A, reads say A
    t[1, :4] = [0., 0., 0.5, 3.5]    # emits G, reads say T: a disagreement of mass 3.5, share 0.875
    t[2, :4] = [1., 1.2, 0., 0.8]    # emits A, heaviest C at share 0.4
    t[1, 4:8] = [0., .5, 0., 0.]
    t[0, 8] = 1.5
    hand = D.Pileup.from_arrays(4, [0], [], np.zeros((0, 3)), t)
    em = b"AGAT"
    assert hand.consensus().tolist() == [0, 3, 1, -1] and hand.depth().tolist() == [6., 4., 3., 0.]
    assert hand.disagreements(em, min_mass=3.0).tolist() == [1]
    assert hand.disagreements(em, min_mass=4.0).tolist() == []
    assert hand.disagreements(em, min_mass=1.0).tolist() == [1]
    assert hand.disagreements(em, min_mass=1.0, min_share=0.39).tolist() == [1, 2]
    assert hand.disagreements(em, min_mass=1.25, min_share=0.39).tolist() == [1]
    assert hand.disagreements(np.frombuffer(b"ATAT", dtype=np.uint8), min_mass=3.0).tolist() == []
    prof = hand.error_profile(em)
    total = 13.0 + 0.5 + 1.5
    assert prof == {"mismatch": (1. + 3.5 + 2.0) / total, "ins": 0.5 / total, "del": 1.5 / total}
    assert D.Pileup.from_arrays(2, [0], [], np.zeros((0, 3)), np.zeros((2, 9))).error_profile(b"AC") == \
        {"mismatch": 0.0, "ins": 0.0, "del": 0.0}
    # the file: an exact round trip, awkward floats included
    t[3] = [1e-310, 0.1 + 0.2, 1 / 3, 5e-324, 1e300, 2.0 ** -1022, 0.0, 7.0, math.pi]
    buf = io.StringIO()
    formats.write_pileup(buf, D.Pileup.from_arrays(4, [0], [], np.zeros((0, 3)), t), em)
    lines = [ln for ln in buf.getvalue().splitlines() if not ln.startswith("#")]
    assert len(lines) == 4 and lines[1].split("\t")[:2] == ["1", "G"] and len(lines[1].split("\t")) == 11
    buf.seek(0)
    em2, t2 = formats.read_pileup(buf)
    assert em2.tobytes() == em and t2.tobytes() == t.tobytes()
    with pytest.raises(ValueError):
        formats.write_pileup(io.StringIO(), hand, b"AGA")


def snp_case():
    """random_genome(120, 3) at k = 8 (126 nodes); six reads hap[s:s + 50], s = 20, 25, .., 45, each with genome position
    60 substituted G -> T -> (arrays, reads)"""
    hap = D.random_genome(120, 3)
    assert chr(hap[60]) == "G"
    arrays = D.vectorised_to_phmm(D.dbg_from_haplotypes([hap], 8), D.PHMMParams.uniform(0.01).with_(n_warmup=8), 0)
    assert arrays.n_nodes == 126
    alt = hap.copy()
    alt[60] = ord("T")
    return arrays, [alt[s:s + 50].tobytes() for s in range(20, 50, 5)]


def test_a_substituted_base_is_one_disagreeing_node(oracle):
    """On the oracle's dense run, every node listed at every position.  Checked there: exactly one node has Match depth
    above 0.5 and a heaviest base other than its emission; it emits G and carries T mass 5.894 of 6; the mismatching
    Match mass over all nodes is 5.8975."""
    arrays, reads = snp_case()
    N = arrays.n_nodes
    om = oracle.Model(arrays)
    sl = []
    with np.errstate(divide="ignore"):
        for r in reads:
            o = om.run(r)
            for p in range(len(r)):
                m, ins, d, _ = o.to_emit_probs(p + 1)
                sl.append(np.stack([m, ins, d], axis=1))
    sl = np.concatenate(sl)
    P = 6 * 50
    read_off = np.arange(7) * 50
    row_off, keys, usage, totals, _ = pileup_ref(read_off, b"".join(reads), np.arange(P + 1) * N, np.tile(np.arange(N), P), sl, N)
    pu = D.Pileup.from_arrays(N, row_off, keys, usage, totals)
    em = CODE[arrays.emission]
    odd = np.nonzero((pu.depth() > 0.5) & (pu.consensus() != em))[0]
    assert odd.size == 1
    v = int(odd[0])
    mismatch = float(sum(pu.match_counts[u, c] for u in range(N) for c in range(4) if c != em[u]))
    print(f"node {v} emits {chr(arrays.emission[v])}: Match by base {pu.match_counts[v].tolist()}; mismatching Match mass "
          f"over all nodes {mismatch:.4f}")
    assert chr(arrays.emission[v]) == "G" and abs(pu.match_counts[v, 3] - 5.894) < 1e-3 and abs(mismatch - 5.8975) < 1e-4
    assert pu.disagreements(arrays.emission, min_mass=3.0).tolist() == [v]
    assert pu.match_counts[v, 3] > 5.5
    prof = pu.error_profile(arrays.emission)
    assert abs(prof["mismatch"] - mismatch / pu.totals.sum()) < 1e-12 and 0.0 < prof["ins"] < 0.01 and 0.0 < prof["del"] < 0.01
