"""GPU: the pileup over mapping lists (phmm_run_with_mapping_pileup, PHMMModel.run_with_mapping_pileup,
include/phmm_amd_pileup.h): per read and (node, read base) the posterior by state, reduced on the device from the values
of the states call, and the per-node totals [N, 9].

The two bars are those of test_gpu_read_usage.py, derived there.
  1. Against the restatement (pileup_ref.py, math.fsum) on the call's OWN states values under the same knobs:
     |got - ref| <= (n + 4) * 2^-52 * ref + n * 2^-1022, n the number of terms; structure and ln P bit for bit; the totals
     against the column sums of the call's own rows by the same bound, n the rows summed (for column 8 the rows of all
     four keys of the node).
  2. Against the oracle (its to_emit_probs(p + 1) at the listed nodes, summed by the same restatement):
     |got - want| <= 1.01e-8 * want + 1.01e-12 * n.
The cross-check against run_with_mapping_read_usage: both calls sum the same terms (the states pass returns the same bits
on repeated calls, the exp is the same function) in different orders; a sum of n non-negative doubles in any order is
within (n - 1) * 2^-53 of the exact sum, so two of them differ by at most (n - 1) * 2^-52 < bar 1 at n, n the list entries
of the node over all reads.

Three cases the issue names cannot be reached on the device.  A read whose LAST list is empty has probability 0 on its
lists (the End state sums the node states of the last list) and is refused by the states half: the crafted read has its
empty lists at the first and a middle position, and the case with the last list empty is held to be that refusal.  A
list that names a node twice is refused by the forward pass of the states half as it stands ("duplicate node in a mapping
list"): the crafted read reaches its 65 terms by 65 listed C positions, and the duplicate is held to be that refusal.  Both
rules -- the position behind an empty last list, a duplicate counting twice -- are covered on the CPU
(test_pileup_ref_cpu.py).  The N > 2^30 - 1 refusal needs a model of more than a thousand million nodes."""
import ctypes as C
import math

import numpy as np
import pytest

import caller_cases as cc
import dbgphmm_amd as D
from dbgphmm_amd import _ffi, _ffi_pileup, _ffi_usage
from dbgphmm_amd.graph import mock_linear_from
from helpers import small_dbg_model, subset_csr
from pileup_ref import pileup_ref
from test_gpu_read_usage import BOTH, GENERIC, _bar1, _bar2, _fixture_reads, _knobs, oracle_states, pad_lists
from test_pileup_ref_cpu import snp_case

pytestmark = pytest.mark.gpu
STATS_USAGE = 2
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731


class _Run:
    """one run_with_mapping_pileup call, its rows on the host, and index 2 of its statistics"""

    def __init__(self, gm, rc, mp, want_totals=True):
        self.lf, self.pu = gm.run_with_mapping_pileup(rc, mp, True, want_totals)
        self.stats = _ffi.last_call_stats(STATS_USAGE)
        self.row_off, self.keys, self.usage = self.pu.arrays()
        self.totals = self.pu.totals if want_totals else None

    def same_bits(self, other):
        return all(cc.same_bits(np.asarray(a), np.asarray(b)) for a, b in
                   ((self.lf, other.lf), (self.row_off, other.row_off), (self.keys, other.keys), (self.usage, other.usage),
                    (self.totals, other.totals)))

    def row(self, r):
        e0, e1 = int(self.row_off[r]), int(self.row_off[r + 1])
        return self.keys[e0:e1], self.usage[e0:e1]


def _chunks(stats, with_totals=True):
    """the chunks of a call from the launches of index 2: the entry offsets, seven per chunk that holds entries and rows
    (keys, sort, heads, scan, starts, sums, row offsets), three behind the totals"""
    n = stats[1] - 1 - (3 if with_totals else 0)
    assert n % 7 == 0, stats
    return n // 7


def _hold(what, run, gm, rc, mp, want_sl=None, usage_of=None):
    """the run against the restatement on the states values of a call under the same knobs (bar 1, structure and ln P bit
    for bit), its totals against its own rows (bar 1), against the oracle's values (bar 2), and against the totals of a
    read-usage call on the same inputs"""
    po, nd, _ = mp.arrays()
    N = gm.n_nodes
    lf, sl, _ = gm.run_with_mapping_states(rc, mp, want_best=False)
    assert cc.same_bits(run.lf, lf), what + ": out_logp_forward is not that of the states call"
    row_off, keys, usage, totals, terms = pileup_ref(rc.offsets, rc.bases, po, nd, sl, N)
    assert np.array_equal(run.row_off, row_off) and np.array_equal(run.keys, keys), what + ": structure"
    assert run.usage.shape == usage.shape and not np.any(np.isnan(run.usage))
    n = terms[:, None].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.nanmax(np.where(usage > 0, np.abs(run.usage - usage) / usage / 2.0 ** -52, 0.0)) if usage.size else 0.0
    print(f"{what}: {keys.size} row entries, segments of 1 .. {int(terms.max()) if terms.size else 0} terms, "
          f"max |got - ref| / ref = {rel:.2f} * 2^-52")
    assert np.all(_bar1(run.usage, usage, n)), what + ": bar 1"
    if run.totals is not None:
        assert run.totals.shape == (N, 9)
        cols = [[[] for _ in range(9)] for _ in range(N)]
        for k, row in zip(run.keys.tolist(), run.usage.tolist()):
            v, c = divmod(k, 4)
            cols[v][c].append(row[0])
            cols[v][4 + c].append(row[1])
            cols[v][8].append(row[2])
        col_ref = np.array([[math.fsum(c) for c in node] for node in cols]).reshape(N, 9)
        col_n = np.array([[len(c) for c in node] for node in cols], dtype=np.float64).reshape(N, 9)
        assert np.array_equal(col_n[:, 8], col_n[:, :4].sum(axis=1))  # column 8: the rows of all four keys
        assert np.all(_bar1(run.totals, col_ref, col_n)), what + ": totals are not the column sums of the rows"
        assert np.all(run.totals[col_n == 0] == 0.0)
        # (against the restatement's totals the rows' own error comes on top, as in test_gpu_read_usage.py)
        assert np.all(_bar1(run.totals, totals, col_n + n.max(initial=0.0))), what + ": totals against the restatement"
    if want_sl is not None:
        _, okeys, want, _, _ = pileup_ref(rc.offsets, rc.bases, po, nd, want_sl, N)
        assert np.array_equal(okeys, keys)
        d = np.abs(run.usage - want)
        print(f"{what}: against the oracle max |d| {float(d.max()) if d.size else 0.0:.3e}")
        assert np.all(_bar2(run.usage, want, n)), what + ": bar 2"
    if usage_of is not None:
        _, u = usage_of
        per_node = np.bincount(nd, minlength=N).astype(np.float64)
        got = np.array([[math.fsum(run.totals[v, 0:4]), math.fsum(run.totals[v, 4:8]), run.totals[v, 8]] for v in range(N)])
        assert np.all(_bar1(got, u.totals, per_node[:, None])), what + ": the totals are not those of the read-usage call"
        # and per read: the nodes of a row are the keys of the read-usage row
        u_off, u_keys, _ = u.arrays()
        for r in range(len(rc)):
            assert np.array_equal(np.unique(run.row(r)[0] >> 2), u_keys[int(u_off[r]):int(u_off[r + 1])])


# ------------------------------------------------------------------ 1. every node listed: the dense run
@pytest.mark.parametrize("which", ["zero_error", "default"])
def test_every_node_listed_is_the_dense_run(gpu_lib, oracle, which):
    """Fails without the feature: the call does not exist."""
    param, read = ((D.PHMMParams.zero_error(), b"CGATC") if which == "zero_error" else (D.PHMMParams.default(), b"ATTCGTCGT"))
    arrays = D.mock_linear().to_phmm(param)
    assert arrays.n_nodes == 10
    gm, rc = D.PHMMModel(arrays), D.ReadCollection([read])
    T = len(read)
    mp = D.Mappings.from_arrays(rc, np.arange(T + 1, dtype=np.uint64) * 10, np.tile(np.arange(10), T))
    po, nd, _ = mp.arrays()
    with np.errstate(divide="ignore"):
        want_sl = oracle_states(oracle, arrays, [read], rc, po, nd)
        run = _Run(gm, rc, mp)
        _hold(f"linear, {which}", run, gm, rc, mp, want_sl, gm.run_with_mapping_read_usage(rc, mp))
    assert run.stats[2] == int(po[-1]) and run.pu.n_nodes == 10 and len(run.pu) == 1
    # a row holds every node under every base the read has
    codes = np.unique(D.model.base_codes(read))
    assert np.array_equal(run.keys, (4 * np.arange(10)[:, None] + codes[None, :]).reshape(-1))
    if which == "zero_error":  # CGATC sits on the nodes 3..7 of ATTCGATCGT, all Match, the read base the emission
        want = np.zeros((10, 9))
        for p, v in enumerate(range(3, 8)):
            want[v, "ACGT".index(chr(read[p]))] = 1.0
        assert np.allclose(run.totals, want, rtol=0.0, atol=1e-12)
        assert run.pu.disagreements(arrays.emission, min_mass=0.5).size == 0
        assert run.pu.consensus()[3:8].tolist() == ["ACGT".index(chr(b)) for b in read]


def test_the_largest_key(gpu_lib, oracle):
    """16 nodes: K = 64 keys; the last node listed at a T base has the key 63 = 4N - 1"""
    seq = b"ATTCGATCGTACGGAT"
    arrays = mock_linear_from(seq).to_phmm(D.PHMMParams.default())
    assert arrays.n_nodes == 16
    read = seq[-6:]
    assert read.endswith(b"T")
    gm, rc = D.PHMMModel(arrays), D.ReadCollection([read])
    T = len(read)
    mp = D.Mappings.from_arrays(rc, np.arange(T + 1, dtype=np.uint64) * 16, np.tile(np.arange(16), T))
    po, nd, _ = mp.arrays()
    with np.errstate(divide="ignore"):
        run = _Run(gm, rc, mp)
        _hold("16 nodes", run, gm, rc, mp, oracle_states(oracle, arrays, [read], rc, po, nd))
    assert int(run.keys.max()) == 63 and int(_ffi_usage.lib().phmm_read_usage_keys(run.pu._h)) == 64
    assert run.totals[15, 3] > 0.9 and run.pu.reads_of(15, 3)[0].tolist() == [0]


# ------------------------------------------------------------------ 2. generated lists
@pytest.fixture(scope="module")
def fix70(gpu_lib, oracle):
    arrays, reads = _fixture_reads(70)
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    with _knobs({}):
        mp, _ = gm.generate_mappings(rc, None, True)
        po, nd, _ = mp.arrays()
        run = _Run(gm, rc, mp)
    return arrays, reads, gm, rc, mp, oracle_states(oracle, arrays, reads, rc, po, nd), run


@pytest.mark.parametrize("n_reads", [1, 5, 70])
def test_generated_lists(gpu_lib, oracle, fix70, n_reads):
    if n_reads == 70:
        arrays, reads, gm, rc, mp, want_sl, run = fix70
    else:
        arrays, reads = _fixture_reads(n_reads)
        gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
        with _knobs({}):
            mp, _ = gm.generate_mappings(rc, None, True)
            run = _Run(gm, rc, mp)
        want_sl = oracle_states(oracle, arrays, reads, rc, *mp.arrays()[:2])
    with _knobs({}):
        _hold(f"generated lists, {n_reads} reads", run, gm, rc, mp, want_sl, gm.run_with_mapping_read_usage(rc, mp))
    po = mp.arrays()[0]
    assert run.stats[1] > 0 and run.stats[2] == int(po[-1]) and _chunks(run.stats) == 1
    assert len(run.pu) == n_reads and run.pu.n_nodes == arrays.n_nodes and run.totals.shape == (arrays.n_nodes, 9)
    # reads_of is the transpose of row
    for key in np.unique(run.keys)[:: max(1, np.unique(run.keys).size // 25)].tolist():
        rd, us = run.pu.reads_of(key >> 2, key & 3)
        assert rd.tolist() == [r for r in range(n_reads) if key in run.row(r)[0]]
        for r, x in zip(rd.tolist(), us):
            keys, usage = run.row(r)
            assert np.array_equal(usage[np.searchsorted(keys, key)], x)
    prof = run.pu.error_profile(arrays.emission)
    print(f"generated lists, {n_reads} reads: error profile {prof}")
    assert all(0.0 <= x < 0.1 for x in prof.values())


# ------------------------------------------------------------------ 3. crafted segments
def _crafted(last_empty=False, twice=False):
    """A 3-mer graph over a read of A, C and one G, every node that emits a base in every list that is not empty.  Read 0:
    its first and a middle list (positions 0 and 2) are empty; the lists that are not lie at exactly 64 A, 65 C and one
    G.  So the fixed node F (as every node) has segments of 64 terms (A: the lane rule at its limit), 65 (C: the wave
    rule), one (G) and no key under T.  Read 1 has one base.  last_empty / twice: the two forms the states half refuses."""
    rng = np.random.default_rng(64)
    body = np.frombuffer(b"A" * 63 + b"C" * 65 + b"G", dtype=np.uint8).copy()
    rng.shuffle(body)
    read0 = b"CAC" + body.tobytes()
    hap = np.frombuffer(read0, dtype=np.uint8)
    sg = D.dbg_from_haplotypes([hap], 3)
    arrays = D.vectorised_to_phmm(sg, D.PHMMParams.uniform(0.01).with_(n_warmup=3), 0)
    real = np.nonzero(D.model.base_codes(arrays.emission) >= 0)[0].tolist()  # (not the pads behind the end)
    F = int(np.argmax(sg.copy_num * (arrays.emission == ord("C"))))  # the C node the read passes most often
    dup = [p for p in range(40, len(read0)) if read0[p:p + 1] == b"C"][0]
    lists = []
    for p in range(len(read0)):
        if p in (0, 2) or (last_empty and p == len(read0) - 1):
            lists.append([])
        else:
            lists.append(real + ([F] if twice and p == dup else []))
    lists.append(real)  # read 1
    reads = [read0, b"A"]
    po = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
    nd = np.concatenate([np.array(x, dtype=np.uint32) for x in lists if x])
    return arrays, reads, po, nd, F, real


def test_crafted_segments(gpu_lib):
    arrays, reads, po, nd, F, real = _crafted()
    N = arrays.n_nodes
    assert N <= 64 and (reads[0].count(b"A"), reads[0].count(b"C"), reads[0].count(b"G"), reads[0].count(b"T")) == (64, 67, 1, 0)
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    mp = D.Mappings.from_arrays(rc, po, nd)
    with _knobs({}):
        run = _Run(gm, rc, mp)
        _hold("crafted segments", run, gm, rc, mp, None, gm.run_with_mapping_read_usage(rc, mp))
        _, sl, _ = gm.run_with_mapping_states(rc, mp, want_best=False)
    _, keys, _, _, terms = pileup_ref(rc.offsets, rc.bases, po, nd, sl, N)
    row0 = {int(k): int(t) for k, t in zip(keys[:int(run.row_off[1])], terms)}
    assert [row0.get(4 * F + c) for c in range(4)] == [64, 65, 1, None]
    assert all([row0.get(4 * v + c) for c in range(4)] == [64, 65, 1, None] for v in real)
    k0, u0 = run.row(0)
    assert k0.size == 3 * len(real) and u0[np.searchsorted(k0, 4 * F + 1), 0] > 1.0  # the 65 terms carry mass
    # the one-base read: every node under A, one term each
    k1, u1 = run.row(1)
    assert np.array_equal(k1, 4 * np.array(real)) and 0.9 < u1[:, 0].sum() + u1[:, 1].sum() < 1.0 + 1e-9  # (InsBegin has the rest)
    # position 1 lies between two empty lists: its entries are dead, and the mass re-enters behind position 2
    assert np.all(sl[:len(real)] == -np.inf) and np.isfinite(run.lf).all()


@pytest.mark.parametrize("form", ["last_empty", "twice"])
def test_an_empty_last_list_and_a_node_listed_twice_are_the_states_refusals(gpu_lib, form):
    arrays, reads, po, nd, F, _ = _crafted(**{form: True})
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    mp = D.Mappings.from_arrays(rc, po, nd)
    out = _Prefilled(2, arrays.n_nodes)
    with _knobs({}):
        assert out.call(gm, rc, mp) == _ffi.PHMM_EINVAL and out.untouched()
        with pytest.raises(D.PhmmError) as e:
            gm.run_with_mapping_states(rc, mp, want_best=False)
        assert e.value.code == _ffi.PHMM_EINVAL


@pytest.mark.parametrize("setting", [GENERIC, BOTH], ids=["generic", "block"])
def test_a_node_that_leaves_the_list(gpu_lib, setting):
    """(as in test_gpu_read_usage.py) every other position p < len-1 of every read gets, at the head of its list, a node
    that list p+1 does not hold: its values are -inf, its terms exact zeros, and its key stays in the row"""
    arrays, _ = small_dbg_model(300, 12, 0.01, seed=5)
    reads = D.sample_reads(arrays, 10 ** 9, 60, seed=5, max_reads=5)
    rc = D.ReadCollection(reads)
    gm = D.PHMMModel(arrays)
    with _knobs({}):
        po, nd, _ = gm.generate_mappings(rc, None, True)[0].arrays()
    po = po.astype(np.int64)
    off = rc.offsets.astype(np.int64)
    rng = np.random.default_rng(6)
    new_off, new, gone = [0], [], []
    for i, r in enumerate(reads):
        for p in range(len(r)):
            g = off[i] + p
            lst = nd[po[g]:po[g + 1]]
            if p % 2 == 0 and p + 1 < len(r):
                pool = np.setdiff1d(np.arange(arrays.n_nodes, dtype=np.uint32), np.concatenate([lst, nd[po[g + 1]:po[g + 2]]]))
                gone.append((i, new_off[-1], int(D.model.base_codes(r[p:p + 1])[0])))
                lst = np.concatenate([[rng.choice(pool)], lst]).astype(np.uint32)
            new.append(lst)
            new_off.append(new_off[-1] + lst.size)
    npo, nnd = np.array(new_off, np.uint64), np.concatenate(new).astype(np.uint32)
    mp = D.Mappings.from_arrays(rc, npo, nnd)
    with _knobs(setting):
        run = _Run(gm, rc, mp)
        _hold("a node leaves the list", run, gm, rc, mp)
        _, sl, _ = gm.run_with_mapping_states(rc, mp, want_best=False)
    assert len(gone) > 100 and all(np.all(sl[a] == -np.inf) for _, a, _ in gone)
    # a key all of whose terms are such entries stays in its row, with exact zeros
    zeros = 0
    for i, a, c in gone:
        key = 4 * int(nnd[a]) + c
        e0, e1 = int(npo[off[i]]), int(npo[off[i + 1]])
        if int(np.sum(nnd[e0:e1] == nnd[a])) == 1:  # (the node is nowhere else in the read's lists)
            keys, usage = run.row(i)
            j = int(np.searchsorted(keys, key))
            assert keys[j] == key and np.all(usage[j] == 0.0) and not np.any(np.signbit(usage[j]))
            zeros += 1
    print(f"a node leaves the list: {zeros} row entries of exact zeros")
    assert zeros > 20


# ------------------------------------------------------------------ 4. wide lists
@pytest.fixture(scope="module")
def wide(gpu_lib):
    """eight reads whose lists are padded to 64, 65, 128, 129, 256, 257, 399 and 400 nodes (pad_lists): 65, 129 and 400
    among them"""
    arrays, _ = small_dbg_model(600, 12, 0.01, seed=3)
    reads = D.sample_reads(arrays, 10 ** 9, 60, seed=4, max_reads=8)
    assert arrays.n_nodes == 740 and len(reads) == 8
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    with _knobs({}):
        po, nd, _ = gm.generate_mappings(rc, None, True)[0].arrays()
    ppo, pnd = pad_lists(po, nd, reads, arrays.n_nodes)
    widths = np.diff(ppo.astype(np.int64))
    assert {65, 129, 400} <= set(widths.tolist())
    return arrays, reads, gm, rc, D.Mappings.from_arrays(rc, ppo, pnd)


@pytest.mark.parametrize("setting", [GENERIC, BOTH], ids=["generic", "block"])
def test_wide_lists(wide, setting):
    arrays, reads, gm, rc, mp = wide
    with _knobs(setting):
        run = _Run(gm, rc, mp)
        _hold("wide lists", run, gm, rc, mp, None, gm.run_with_mapping_read_usage(rc, mp))
    assert run.stats[2] == int(mp.arrays()[0][-1])


# ------------------------------------------------------------------ 5. seams, independence
def test_seams(gpu_lib, fix70):
    """the 70 reads with the lists of the longest of the reads 10..59 padded to 300 nodes, so that it holds more entries
    than any cap the limit leaves: it is a chunk of its own, with chunks of several reads before and behind it"""
    arrays, reads, gm, rc, mp, _, _ = fix70
    N = arrays.n_nodes
    assert N > 300
    po, nd, _ = mp.arrays()
    po = po.astype(np.int64)
    off = rc.offsets.astype(np.int64)
    rng = np.random.default_rng(35)
    B = 10 + int(np.argmax([len(r) for r in reads[10:60]]))
    new_off, new = [0], []
    for g in range(int(off[-1])):
        lst = nd[po[g]:po[g + 1]]
        if off[B] <= g < off[B + 1]:
            others = np.setdiff1d(np.arange(N, dtype=np.uint32), lst)
            lst = np.concatenate([lst, rng.choice(others, size=300 - lst.size, replace=False).astype(np.uint32)])
        new.append(lst)
        new_off.append(new_off[-1] + lst.size)
    npo, nnd = np.array(new_off, np.uint64), np.concatenate(new).astype(np.uint32)
    mp2 = D.Mappings.from_arrays(rc, npo, nnd)
    per_read = (npo[off[1:]] - npo[off[:-1]]).astype(np.int64)
    n_ent, big = int(npo[-1]), int(per_read[B])
    rest = np.delete(per_read, B)
    assert big == 300 * len(reads[B]) and big > 8 * int(rest.max())
    with _knobs({}):
        full = _Run(gm, rc, mp2)
        assert _chunks(full.stats) == 1
        # the plane, the reads' first entries and the scratch (the header: 32 bytes per list entry of a chunk and about
        # 12 of the sort's own) of 0.6 of that read: the cap lies below it and above two of any other reads
        _ffi.check(gpu_lib.phmm_set_workspace_limit(24 * n_ent + 8 * 71 + 44 * (6 * big // 10) + (64 << 10)))
        try:
            split = _Run(gm, rc, mp2)
        finally:
            _ffi.check(gpu_lib.phmm_set_workspace_limit(0))
        chunks = _chunks(split.stats)
        print(f"seams: read {B} holds {big} of {n_ent} entries; {chunks} chunks under the limit")
        assert chunks >= 3 and split.stats[2] == n_ent
        assert split.same_bits(full)
        _hold("seams", split, gm, rc, mp2)
        # the limit is restored: one chunk again
        assert _chunks(_Run(gm, rc, mp2).stats) == 1


def test_independence(gpu_lib, fix70):
    arrays, reads, gm, rc, mp, _, full = fix70
    po, nd, _ = mp.arrays()
    off = rc.offsets.astype(np.int64)
    with _knobs({}):
        pick = [3, 3, 7, 69]  # the same read twice in a row: two rows, not one merged segment
        rc2 = D.ReadCollection([reads[j] for j in pick])
        mp2 = D.Mappings.from_arrays(rc2, *subset_csr(off, (po, nd, np.zeros(nd.size)), pick)[:2])
        sub = _Run(gm, rc2, mp2)
        for j, r in enumerate(pick):
            assert np.array_equal(sub.row(j)[0], full.row(r)[0]) and cc.same_bits(sub.row(j)[1], full.row(r)[1])
            assert sub.lf[j] == full.lf[r]
        again = _Run(gm, rc, mp)
        assert again.same_bits(full) and again.stats[1:] == full.stats[1:]


# ------------------------------------------------------------------ 6. output forms
def test_output_forms(gpu_lib, fix70):
    """every combination of NULL, host and device outputs gives the same bits; out == NULL and want_rows=False work; the
    rows leave through phmm_read_usage_export; a call without reads writes nothing and returns a handle of 0 rows"""
    arrays, reads, gm, rc, mp, _, full = fix70
    L = _ffi_pileup.lib()
    R, N, T = len(reads), arrays.n_nodes, int(full.keys.size)
    with _knobs({}):
        for lf_form in ("null", "host", "device"):
            for tot_form in ("null", "host", "device"):
                for with_handle in (False, True):
                    lf_h, tot_h = np.full(R, 7.5), np.full((N, 9), 7.5)
                    dl, dt = cc.DeviceArray(8 * R, slack=cc.SLACK), cc.DeviceArray(72 * N, slack=cc.SLACK)
                    h = C.c_void_p()
                    _ffi.check(L.phmm_run_with_mapping_pileup(
                        gm._h, rc._h, mp._h, {"null": None, "host": P(lf_h), "device": dl.p}[lf_form],
                        {"null": None, "host": P(tot_h), "device": dt.p}[tot_form], C.byref(h) if with_handle else None))
                    try:
                        what = (lf_form, tot_form, with_handle)
                        if lf_form != "null":
                            assert cc.same_bits(lf_h if lf_form == "host" else dl.numpy(np.float64), full.lf), what
                        if tot_form != "null":
                            got = tot_h if tot_form == "host" else dt.numpy(np.float64).reshape(N, 9)
                            assert cc.same_bits(got, full.totals), what
                        assert np.all(dl.bytes()[8 * R:] == cc.POISON) and np.all(dt.bytes()[72 * N:] == cc.POISON), what
                        if lf_form != "device":
                            assert np.all(dl.bytes() == cc.POISON)
                        if tot_form != "device":
                            assert np.all(dt.bytes() == cc.POISON)
                        if with_handle:
                            U = _ffi_usage.lib()
                            assert (U.phmm_read_usage_reads(h), U.phmm_read_usage_keys(h), U.phmm_read_usage_total(h)) == (R, 4 * N, T)
                            row_off, keys, usage = np.zeros(R + 1, np.uint64), np.zeros(T, np.uint32), np.zeros((T, 3))
                            _ffi.check(U.phmm_read_usage_export(h, P(row_off), P(keys), P(usage)))
                            assert np.array_equal(row_off, full.row_off) and np.array_equal(keys, full.keys), what
                            assert cc.same_bits(usage, full.usage), what
                    finally:
                        _ffi_usage.lib().phmm_read_usage_destroy(h)
                        dl.free()
                        dt.free()
        # the export into device memory
        h = C.c_void_p()
        _ffi.check(L.phmm_run_with_mapping_pileup(gm._h, rc._h, mp._h, None, None, C.byref(h)))
        try:
            d_off, d_keys, d_use = (cc.DeviceArray(8 * (R + 1), slack=cc.SLACK), cc.DeviceArray(4 * T, slack=cc.SLACK),
                                    cc.DeviceArray(24 * T, slack=cc.SLACK))
            _ffi.check(_ffi_usage.lib().phmm_read_usage_export(h, d_off.p, d_keys.p, d_use.p))
            assert np.array_equal(d_off.numpy(np.uint64), full.row_off) and np.array_equal(d_keys.numpy(np.uint32), full.keys)
            assert cc.same_bits(d_use.numpy(np.float64).reshape(T, 3), full.usage)
            assert all(np.all(d.bytes()[d.nbytes:] == cc.POISON) for d in (d_off, d_keys, d_use))
        finally:
            _ffi_usage.lib().phmm_read_usage_destroy(h)
        # the Python forms
        lf, no_rows = gm.run_with_mapping_pileup(rc, mp, want_rows=False)
        assert cc.same_bits(lf, full.lf) and cc.same_bits(no_rows.totals, full.totals) and no_rows._h is None
        with pytest.raises(ValueError):
            no_rows.arrays()
        alone = _Run(gm, rc, mp, want_totals=False)
        assert alone.totals is None and np.array_equal(alone.keys, full.keys) and cc.same_bits(alone.usage, full.usage)
        # (the totals summed on the host from the rows: another order, so to rounding)
        assert np.allclose(alone.pu.totals, full.totals, rtol=1e-12, atol=0.0)
        # no reads: nothing is written, the handle has 0 rows
        rc0 = D.ReadCollection([])
        mp0 = D.Mappings.from_arrays(rc0, np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint32))
        lf, tot = np.full(1, 7.5), np.full((N, 9), 7.5)
        h = C.c_void_p()
        _ffi.check(L.phmm_run_with_mapping_pileup(gm._h, rc0._h, mp0._h, P(lf), P(tot), C.byref(h)))
        try:
            U = _ffi_usage.lib()
            assert h.value and np.all(lf == 7.5) and np.all(tot == 7.5)
            assert (U.phmm_read_usage_reads(h), U.phmm_read_usage_keys(h), U.phmm_read_usage_total(h)) == (0, 4 * N, 0)
            row_off = np.full(1, 9, dtype=np.uint64)
            _ffi.check(U.phmm_read_usage_export(h, P(row_off), None, None))
            assert row_off.tolist() == [0]
        finally:
            _ffi_usage.lib().phmm_read_usage_destroy(h)
        lf0, p0 = gm.run_with_mapping_pileup(rc0, mp0)
        assert lf0.size == 0 and len(p0) == 0 and p0.arrays()[1].size == 0 and np.all(p0.totals == 0.0)


# ------------------------------------------------------------------ 7. refusals
class _Prefilled:
    """outputs of a raw call, pre-filled, and a handle slot that holds a mark: a refusal leaves them as they are"""
    MARK = 0x1234560

    def __init__(self, n_reads, n_nodes):
        self.lf, self.tot = np.full(max(n_reads, 1), 7.5), np.full((max(n_nodes, 1), 9), 7.5)
        self.h = C.c_void_p(self.MARK)

    def call(self, gm, rc, mp):
        return _ffi_pileup.lib().phmm_run_with_mapping_pileup(gm._h, rc._h, mp._h, P(self.lf), P(self.tot), C.byref(self.h))

    def untouched(self):
        return bool(np.all(self.lf == 7.5) and np.all(self.tot == 7.5) and self.h.value == self.MARK)


@pytest.mark.parametrize("bad", [b"N", b"a", b"t"])
def test_a_byte_that_is_no_base_is_refused(gpu_lib, fix70, bad):
    arrays, reads, gm, rc, mp, _, full = fix70
    po, nd, _ = mp.arrays()
    r, p = 41, 17
    spoiled = list(reads)
    spoiled[r] = reads[r][:p] + bad + reads[r][p + 1:]
    rc2 = D.ReadCollection(spoiled)
    mp2 = D.Mappings.from_arrays(rc2, po, nd)
    out = _Prefilled(len(reads), arrays.n_nodes)
    with _knobs({}):
        assert out.call(gm, rc2, mp2) == _ffi.PHMM_EINVAL and out.untouched()
        msg = gpu_lib.phmm_last_error().decode()
        assert f"read {r}" in msg and f"position {p}" in msg, msg
        with pytest.raises(D.PhmmError) as e:
            gm.run_with_mapping_pileup(rc2, mp2)
        assert e.value.code == _ffi.PHMM_EINVAL
        assert _Run(gm, rc, mp).same_bits(full)  # and the call still works


def test_refusals_of_the_states_and_usage_calls(gpu_lib, wide, fix70):
    """(the N > 2^30 - 1 refusal cannot be reached in a test: it needs a model of more than a thousand million nodes)"""
    arrays, reads, gm, rc_all, mp_all = wide
    ppo, pnd, _ = mp_all.arrays()
    N = arrays.n_nodes
    rc2 = D.ReadCollection(reads[:2])
    n = len(reads[0]) + len(reads[1])
    # every node listed at bases 30..35 of read 7 (lists of 400 nodes) goes to copy number 0: the read is cut there
    _, sg = small_dbg_model(600, 12, 0.01, seed=3)
    p0 = int(rc_all.offsets[7])
    cn = sg.copy_num.copy()
    cn[np.unique(pnd[int(ppo[p0 + 30]):int(ppo[p0 + 36])])] = 0
    with np.errstate(divide="ignore"):
        a2 = D.vectorised_to_phmm(D.SeqGraph(cn, sg.base, sg.edge_src, sg.edge_dst, None), arrays.param, 0)
    cut = D.PHMMModel(a2)

    def list_of_401(out):  # (refused where the lists are handed over, as for the states call)
        try:
            over = D.Mappings.from_arrays(rc2, np.arange(n + 1, dtype=np.uint64) * 401, np.tile(np.arange(401, dtype=np.uint32), n))
        except D.PhmmError as e:
            return e.code
        return out.call(gm, rc2, over)

    def node_out_of_range(out):
        try:
            over = D.Mappings.from_arrays(rc2, np.arange(n + 1, dtype=np.uint64), np.full(n, N, dtype=np.uint32))
        except D.PhmmError as e:
            return e.code
        return out.call(gm, rc2, over)

    for setting in (BOTH, GENERIC):
        with _knobs(setting):
            outs = [_Prefilled(2, N), _Prefilled(2, N), _Prefilled(8, N), _Prefilled(2, N)]
            got = (outs[0].call(gm, rc2, mp_all), list_of_401(outs[1]), outs[2].call(cut, rc_all, mp_all), node_out_of_range(outs[3]))
            assert got == (_ffi.PHMM_EINVAL, _ffi.PHMM_ECAPACITY, _ffi.PHMM_EINVAL, _ffi.PHMM_EINVAL), got
            assert all(o.untouched() for o in outs)
    L = _ffi_pileup.lib()
    for args in ((None, rc2._h, mp_all._h), (gm._h, None, mp_all._h), (gm._h, rc2._h, None)):
        assert L.phmm_run_with_mapping_pileup(*args, None, None, None) == _ffi.PHMM_EINVAL
    # the plane alone does not fit the workspace limit: refused as the read-usage call refuses
    arrays70, reads70, gm70, rc70, mp70, _, full = fix70
    n_ent = int(mp70.arrays()[0][-1])
    out = _Prefilled(70, arrays70.n_nodes)
    with _knobs({}):
        _ffi.check(gpu_lib.phmm_set_workspace_limit(24 * n_ent - 8))
        try:
            assert out.call(gm70, rc70, mp70) == _ffi.PHMM_ECAPACITY and out.untouched()
        finally:
            _ffi.check(gpu_lib.phmm_set_workspace_limit(0))
        assert _Run(gm70, rc70, mp70).same_bits(full)


# ------------------------------------------------------------------ 8. the caller contract
@pytest.fixture(scope="module")
def ctx(gpu_lib):
    return cc.Ctx()


@pytest.fixture(scope="module")
def scratch(gpu_lib):
    s = cc.DeviceArray(cc.SCRATCH_BYTES, 0)
    yield s
    s.free()


def _exported(h):
    U = _ffi_usage.lib()
    R, T = U.phmm_read_usage_reads(h), U.phmm_read_usage_total(h)
    row_off, keys, usage = np.zeros(R + 1, dtype=np.uint64), np.zeros(max(T, 1), dtype=np.uint32), np.zeros((max(T, 1), 3))
    _ffi.check(U.phmm_read_usage_export(h, P(row_off), P(keys), P(usage)))
    return {"row_off": row_off, "keys": keys[:T], "usage": usage[:T]}


def _row():
    """the new entry point as a row of caller_cases: the two output arrays where the caller wants them, the handle
    exported through the host-pointer form into extras"""
    L = _ffi_pileup.lib()
    outs = lambda c: [cc.Out("logp_forward", cc.F8, (c.R,)), cc.Out("node_pileup", cc.F8, (c.N, 9))]  # noqa: E731

    def call(c, b):
        h = C.c_void_p()
        c.ffi.check(L.phmm_run_with_mapping_pileup(c.gm._h, c.rc._h, c.mp._h, b["logp_forward"], b["node_pileup"], C.byref(h)))
        try:
            return _exported(h)
        finally:
            _ffi_usage.lib().phmm_read_usage_destroy(h)
    return cc.Row("run_with_mapping_pileup", list(_ffi_pileup.PILEUP_SYMBOLS["phmm_amd_pileup.h"]), outs, call)


def test_device_outputs_and_a_busy_stream(ctx, scratch):
    row = _row()
    want = cc.run_host(ctx, row)
    assert np.all(np.isfinite(want["logp_forward"])) and want["keys"].size > 0 and np.any(want["node_pileup"] > 0)
    for stream in (None, cc.Stream()):
        d = cc.DeviceOutputs(ctx, row, stream)
        try:
            if stream is None:
                extras = row.call(ctx, d.pointers())
                got, clean = d.read()
            else:
                with cc.on_stream(ctx.lib, stream):
                    cc.queue_work(stream, scratch)
                    d.poison(stream)
                    busy = stream.query()
                    extras = row.call(ctx, d.pointers())
                    got, clean = d.read()
                assert busy == cc.HIP_ERROR_NOT_READY, "the queued work had drained before the call: the case ordered nothing"
            got.update(extras)
            assert not cc.same_result(want, got), cc.same_result(want, got)
            assert set(want) == set(got) and clean, "bytes behind an output's extent were written"
        finally:
            d.free()
            if stream is not None:
                stream.destroy()


def test_two_streams_alternating(ctx):
    row = _row()
    want = cc.run_host(ctx, row)
    streams = [cc.Stream(), cc.Stream()]
    try:
        for k in range(4):
            with cc.on_stream(ctx.lib, streams[k % 2]):
                got = cc.run_host(ctx, row)
            assert not cc.same_result(want, got), (k, cc.same_result(want, got))
    finally:
        for s in streams:
            s.destroy()


def test_four_calls_do_not_grow_the_workspace(ctx):
    row = _row()
    runs, ws = [], []
    for _ in range(4):
        runs.append(cc.run_host(ctx, row))
        ws.append(ctx.lib.phmm_workspace_bytes())
    assert ws[1] == ws[2] == ws[3], ws
    for k in (1, 2, 3):
        assert not cc.same_result(runs[0], runs[k]), (k, cc.same_result(runs[0], runs[k]))


def test_the_handle_outlives_its_inputs(gpu_lib):
    """exported after the model, the reads and the mappings are destroyed: the handle borrows nothing"""
    arrays, reads = _fixture_reads(5)
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    with _knobs({}):
        mp, _ = gm.generate_mappings(rc, None, True)
        want = _Run(gm, rc, mp)
        lf, pu = gm.run_with_mapping_pileup(rc, mp)
    del mp, rc, gm
    import gc
    gc.collect()
    other = D.PHMMModel(D.mock_linear().to_phmm(D.PHMMParams.default()))  # (another model takes the device meanwhile)
    other.run(b"ATTCGTCGT")
    row_off, keys, usage = pu.arrays()
    assert np.array_equal(row_off, want.row_off) and np.array_equal(keys, want.keys) and cc.same_bits(usage, want.usage)


# ------------------------------------------------------------------ 9. the substituted base
def test_a_substituted_base_is_one_disagreeing_node(gpu_lib):
    """the case of test_pileup_ref_cpu.py on lists from generate_mappings: six reads over genome position 60 with G -> T
    make exactly the node that emits that G disagree, its T column above 5.5 of 6"""
    arrays, reads = snp_case()
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    with _knobs({}):
        mp, _ = gm.generate_mappings(rc, None, True)
        run = _Run(gm, rc, mp)
        _hold("substituted base", run, gm, rc, mp)
    found = run.pu.disagreements(arrays.emission, min_mass=3.0)
    assert found.tolist() == [60] and chr(arrays.emission[60]) == "G"
    print(f"substituted base: node 60 Match by base {run.pu.match_counts[60].tolist()}")
    assert run.pu.match_counts[60, 3] > 5.5
    rd, us = run.pu.reads_of(60, 3)
    assert rd.tolist() == list(range(6)) and np.all(us[:, 0] > 0.9)
