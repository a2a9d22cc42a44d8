"""CPU: the Python restatement of posterior path sampling over mapping lists (tests/sample_paths_ref.py) stands on its
own before it judges a kernel.
  1. its ln Z is the oracle's forward total over the same lists (as sets) within 1e-9, the slack
     tests/test_gpu_best_path.py gives the same oracle quantity;
  2. 40 000 walks of a read follow the exact law: chi-square of the path counts against N exp(value - ln Z), paths scored
     by best_path_ref.score_path, bar df + 5 sqrt(2 df);
  3. on 3-node integer-log models every legal path is enumerated from the model alone: the weights sum to exp(ln Z),
     every sampled path is one of them, a single decision's choice frequencies match its weights, and a list that names
     a node twice gives the ln Z and the walks of the list without the duplicate;
  4. no decision of a fixture the GPU test compares word for word has a margin below 1e-9 (a condition on the inputs:
     a fixture that fails it gets another seed in sample_paths_ref.SEEDS, never another threshold);
  5. the sampled frequency of every emitting state on dbg x 16 copies agrees with the oracle's state posterior within
     6 binomial standard deviations plus 1 / N (the GPU test asserts the same of the kernel's samples, same seeds)."""
import math

import numpy as np
import pytest

import dbgphmm_amd as D
import best_path_ref as B
import sample_paths_ref as S

NINF = -math.inf


def _as_set(lst):
    """the list without its later duplicates"""
    seen, out = set(), []
    for v in lst:
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


# ---------------------------------------------------------------- 1. ln Z against the oracle
@pytest.mark.parametrize("graph", ["dbg", "zoo"])
def test_logz_is_the_oracles_forward_total(oracle, graph):
    b = S.base_case(graph)
    reads = b["reads"]
    lists = S._oracle_lists(b["arrays"], reads)
    om = oracle.Model(b["arrays"])
    worst = 0.0
    for r, ls in zip(reads, lists):
        want = om.forward_score_only(r, oracle.Mapping.from_lists(ls))
        got = S.forward(b["arrays"], r, ls).logz
        worst = max(worst, abs(got - want))
    print(f"{graph}: {len(reads)} reads, |ln Z - forward_score_only| at most {worst:.3e}")
    assert worst <= 1e-9


def test_logz_of_every_fixture(oracle):
    worst = 0.0
    for k, f in enumerate(S.fixtures()):
        om = oracle.Model(f["arrays"])
        for j, (r, ls) in enumerate(zip(f["reads"], f["lists"])):
            want = om.forward_score_only(r, oracle.Mapping.from_lists([_as_set(x) for x in ls]))
            got = S.fixture_samples(k)[j]["logz"]
            if want == NINF or got == NINF:
                assert got == want, (f["tag"], j, got, want)
                continue
            worst = max(worst, abs(got - want))
            assert abs(got - want) <= 1e-9, (f["tag"], j, got, want)
    print(f"all fixtures: |ln Z - forward_score_only| at most {worst:.3e}")


# ---------------------------------------------------------------- 2. the exact law by brute force
@pytest.mark.parametrize("read", S.CHI_READS)
def test_chi_square_of_sampled_paths(read):
    arrays, _ = S.chi_case()
    ls = S.full_lists(arrays, read)
    res = S.sample_set(arrays, [read] * S.CHI_COPIES, [ls] * S.CHI_COPIES, S.CHI_SAMPLES, S.CHI_SEED)
    walks = [r["rows"][s] for r in res for s in range(S.CHI_SAMPLES)]
    assert len(walks) == 40000
    chi, df, distinct = S.chi_square(arrays, read, ls, res[0]["logz"], walks)
    print(f"{read}: {distinct} distinct paths, chi-square {chi:.1f} at df {df}, bar {S.chi_bar(df):.1f}")
    assert df >= 50 and chi <= S.chi_bar(df)


# ---------------------------------------------------------------- 3. the rules by enumeration
def tiny_int(gaps, seed):
    """3 nodes, 3 to 5 edges and one of them twice, small integer logs with some -inf, a read of 3 bases over two letters,
    lists of 1 to 3 distinct entries (1 or 2 at n_max_gaps = 2)"""
    rng = np.random.default_rng([20261023, seed])

    def logs(n, p_inf):
        return np.where(rng.random(n) < p_inf, NINF, rng.choice([0.0, -1.0, -2.0], size=n))
    names = ["p_mismatch", "p_match", "p_random", "p_gap_open", "p_gap_ext", "p_end", "p_MM", "p_IM", "p_DM", "p_MI",
             "p_II", "p_DI", "p_MD", "p_ID", "p_DD"]
    p = B.int_params(gaps, **dict(zip(names, logs(15, 0.05).tolist())))
    pairs = [(u, v) for u in range(3) for v in range(3)]
    e = [pairs[i] for i in rng.choice(9, size=int(rng.integers(3, 6)), replace=False)]
    e.append(e[0])
    e = np.array(e, dtype=np.uint32)
    arrays = D.PHMMArrays(p, rng.choice(np.frombuffer(b"AC", dtype=np.uint8), size=3), logs(3, 0.15), e[:, 0].copy(),
                          e[:, 1].copy(), logs(len(e), 0.1))
    read = bytes(rng.choice(np.frombuffer(b"AC", dtype=np.uint8), size=3))
    lists = [rng.permutation(3)[:int(rng.integers(1, 4 if gaps < 2 else 3))].tolist() for _ in range(3)]
    return arrays, read, lists


def enumerate_paths(arrays, read, lists):
    """every path of the model over lists WITHOUT duplicates -> {rows as bytes: (rows, ln weight)}.  Written from the
    model alone: per base an emitting state (InsBegin while no node state has been seen; Match of a listed node, from
    Begin / InsBegin by init or over every edge from the node stood on; Ins of the node stood on if it is listed) and then
    0 to G + 1 Dels over edges within the list (from InsBegin by init).  Parallel edges add their weights."""
    p = arrays.param
    G, L = int(p.n_max_gaps), len(read)
    init, emis = arrays.init_logp.tolist(), arrays.emission.tolist()
    w_edge = {}
    for u, v, t in zip(arrays.edge_src.tolist(), arrays.edge_dst.tolist(), arrays.trans_logp.tolist()):
        w_edge[(u, v)] = w_edge.get((u, v), 0.0) + math.exp(t)

    def ln(x):
        return math.log(x) if x > 0.0 else NINF
    to = {("B", "M"): p.p_MM, ("IB", "M"): p.p_IM, ("M", "M"): p.p_MM, ("I", "M"): p.p_IM, ("D", "M"): p.p_DM,
          ("B", "I"): p.p_MI, ("IB", "I"): p.p_II, ("M", "I"): p.p_MI, ("I", "I"): p.p_II, ("D", "I"): p.p_DI,
          ("IB", "D"): p.p_ID, ("M", "D"): p.p_MD, ("I", "D"): p.p_ID, ("D", "D"): p.p_DD}
    out = {}

    def dels(pos, kind, node, left, row, value, rows):
        done = rows + [row + [S.NONE] * (G + 2 - len(row))]
        step(pos + 1, kind, node, value, done)
        if left == 0:
            return
        for s, w in enumerate(lists[pos]):
            e = init[w] if kind == "IB" else ln(w_edge.get((node, w), 0.0))
            v = value + e + to[(kind, "D")]
            if v > NINF:
                dels(pos, "D", w, left - 1, row + [(s << 2) | 2], v, rows)

    def step(pos, kind, node, value, rows):
        if pos == L:
            if kind not in ("B", "IB") and value + p.p_end > NINF:
                out[np.array(rows, dtype=np.uint32).tobytes()] = (np.array(rows, dtype=np.uint32), value + p.p_end)
            return
        if kind in ("B", "IB"):
            v = value + to[(kind, "I")] + p.p_random
            if v > NINF:
                dels(pos, "IB", None, G + 1, [S.INS_BEGIN], v, rows)
        for s, w in enumerate(lists[pos]):
            e = init[w] if kind in ("B", "IB") else ln(w_edge.get((node, w), 0.0))
            v = value + e + to[(kind, "M")] + (p.p_match if emis[w] == read[pos] else p.p_mismatch)
            if v > NINF:
                dels(pos, "M", w, G + 1, [(s << 2) | 0], v, rows)
            if kind not in ("B", "IB") and w == node:
                v = value + to[(kind, "I")] + p.p_random
                if v > NINF:
                    dels(pos, "I", w, G + 1, [(s << 2) | 1], v, rows)
    step(0, "B", None, 0.0, [])
    return out


N_TINY = 24


@pytest.fixture(scope="module")
def tiny_runs():
    """-> [(arrays, read, lists, paths, Forward)] over N_TINY random cases, n_max_gaps 0, 1, 2 in turn"""
    out = []
    for seed in range(N_TINY):
        arrays, read, lists = tiny_int(seed % 3, seed)
        out.append((arrays, read, lists, enumerate_paths(arrays, read, lists), S.forward(arrays, read, lists)))
    return out


def test_path_weights_sum_to_one(tiny_runs):
    finite = 0
    for seed, (arrays, read, lists, paths, F) in enumerate(tiny_runs):
        if not paths:
            assert F.logz == NINF, seed
            continue
        finite += 1
        total = sum(math.exp(v - F.logz) for _, v in paths.values())
        assert abs(total - 1.0) <= 1e-12 * max(len(paths), 1), (seed, total, len(paths))
    print(f"{finite} of {N_TINY} cases have a path")
    assert finite >= N_TINY // 2


def test_sampled_paths_are_legal_and_follow_the_weights(tiny_runs):
    """every walk is one of the enumerated paths, and over 64 x 40 walks per case the path counts pass the chi-square of
    section 2 against the enumerated weights"""
    tested = 0
    for seed, (arrays, read, lists, paths, F) in enumerate(tiny_runs):
        if not paths:
            continue
        walks = []
        for r in range(40):
            res = S.sample_read(arrays, read, lists, r, 64, 100 + seed, F)
            walks += list(res["rows"])
        seen = {}
        for rows in walks:
            key = rows.tobytes()
            assert key in paths, (seed, rows.tolist())
            seen[key] = seen.get(key, 0) + 1
        N = len(walks)
        chi, cells, big_n, big_e = 0.0, 0, 0, 0.0
        for key, (_, v) in paths.items():
            e = N * math.exp(v - F.logz)
            if e >= 5.0:
                chi += (seen.get(key, 0) - e) ** 2 / e
                cells, big_n, big_e = cells + 1, big_n + seen.get(key, 0), big_e + e
        if N - big_e > 1e-9 * N:
            chi += ((N - big_n) - (N - big_e)) ** 2 / (N - big_e)
            cells += 1
        if cells >= 2:
            tested += 1
            assert chi <= S.chi_bar(cells - 1), (seed, chi, cells - 1)
    assert tested >= 8


def test_single_decision_frequencies():
    """the draw rule on its own: 20 000 draws of one decision against its weights, -inf and underflowing candidates never
    chosen, the single candidate always"""
    terms = [-1.0, NINF, -3.0, -0.5, -2000.0, -2.0]
    _, w = S.weights(terms)
    total = sum(w)
    n = 20000
    count = [0] * len(terms)
    x0 = S.stream(3, 0, 0)
    for d in range(1, n + 1):
        c, margin = S.draw(terms, S.uniform(x0, d))
        count[c] += 1
        assert margin >= 0.0
    assert count[1] == 0 and count[4] == 0
    for i, x in enumerate(w):
        prob = x / total
        assert abs(count[i] / n - prob) <= S.binomial_bar(prob, n), (i, count[i], prob)
    assert S.draw([NINF, -7.0, NINF], 0.999999)[0] == 1 and S.draw([-7.0], 0.0) == (0, math.inf)
    assert S.draw([NINF, NINF], 0.5)[0] is None
    # the boundary belongs to the later candidate (u * c_last < c_i is strict), and rounding at the top falls back
    assert S.draw([0.0, 0.0], 0.5)[0] == 1 and S.draw([0.0, 0.0], 0.49999)[0] == 0
    assert S.draw([0.0, NINF], 1.0)[0] == 0


def test_the_stream_is_the_headers():
    """SplitMix64's finaliser on known inputs, and u in [0, 1) with 53 bits"""
    # (the first two outputs of SplitMix64 seeded with 0, the published test vector)
    assert S.mix(0) == 0 and S.mix(S.GOLD) == 0xE220A8397B1DCDAF and S.mix(2 * S.GOLD) == 0x6E789E6AA1B965F4
    x0 = S.stream(7, 3, 5)
    assert x0 == S.mix(7 ^ S.mix(3 * 64 + 5 + S.GOLD))
    us = [S.uniform(x0, d) for d in range(1, 1001)]
    assert all(0.0 <= u < 1.0 and u * 2.0 ** 53 == int(u * 2.0 ** 53) for u in us)
    assert 0.45 < sum(us) / len(us) < 0.55 and len(set(us)) == len(us)


def test_duplicate_rule(tiny_runs):
    """a list that names a node twice: the ln Z of the list without the duplicate, and the same walks up to the slot
    numbering (a later duplicate holds no state, so the slots behind it move by one)"""
    tested = 0
    for seed, (arrays, read, lists, paths, F) in enumerate(tiny_runs):
        if not paths:
            continue
        for where in ("behind", "inside"):
            dup = []
            for lst in lists:
                dup.append(lst + [lst[0]] if where == "behind" else [lst[0], lst[0]] + lst[1:])
            Fd = S.forward(arrays, read, dup)
            assert Fd.logz == F.logz, (seed, where)
            a = S.sample_read(arrays, read, lists, 5, 16, seed, F)
            b = S.sample_read(arrays, read, dup, 5, 16, seed, Fd)
            want = a["rows"].copy()
            if where == "inside":  # every slot >= 1 moves by one
                node = (want != S.NONE) & (want != S.INS_BEGIN)
                want[node & ((want >> 2) >= 1)] += np.uint32(1 << 2)
            assert np.array_equal(b["rows"], want), (seed, where)
            assert np.array_equal(a["counts"], b["counts"]) and np.array_equal(a["path_logp"], b["path_logp"])
            tested += 1
    assert tested >= N_TINY


# ---------------------------------------------------------------- 4. the margins of the shared fixtures
def test_no_decision_of_a_fixture_is_near_a_boundary():
    smallest, n_paths = math.inf, 0
    for k, f in enumerate(S.fixtures()):
        res = S.fixture_samples(k)
        m = min(r["margin"] for r in res)
        smallest = min(smallest, m)
        n_paths += sum(f["n_samples"] for r in res if r["logz"] > NINF)
        assert m >= S.MIN_MARGIN, (f["tag"], f["seed"], m)
    print(f"{n_paths} walks over {len(S.fixtures())} fixtures: the smallest margin is {smallest:.3e}")
    c = S.consistency_case()
    assert min(r["margin"] for r in _consistency_samples()) >= S.MIN_MARGIN, c["tag"]


def test_fixture_walks_rescore_to_their_own_terms():
    """score_path accepts every walk, counts what the walk counted, and its value is the walk's own sum within the bar
    once the lighter parallel edges are accounted for"""
    lighter = 0
    for k, f in enumerate(S.fixtures()):
        for j, (r, ls) in enumerate(zip(f["reads"], f["lists"])):
            res = S.fixture_samples(k)[j]
            if res["logz"] == NINF:
                assert np.all(res["rows"] == S.NONE) and np.all(res["path_logp"] == NINF) and not res["counts"].any()
                continue
            for s in range(f["n_samples"]):
                v, n_terms, cnt = S.score_path(f["arrays"], r, ls, res["rows"][s])
                assert cnt == res["counts"][s].tolist()
                assert abs(v + res["corr"][s] - res["path_logp"][s]) <= S.bar(n_terms, v), (f["tag"], j, s)
                assert res["path_logp"][s] <= res["logz"] + S.bar(n_terms, v)
                lighter += res["corr"][s] != 0.0
    print(f"{lighter} walks take the lighter of two parallel edges somewhere")


# ---------------------------------------------------------------- 5. against the state posteriors
@pytest.fixture(scope="module")
def consistency_samples():
    return _consistency_samples()


_CACHE = {}


def _consistency_samples():
    if "c" not in _CACHE:
        c = S.consistency_case()
        _CACHE["c"] = S.sample_set(c["arrays"], c["reads"], c["lists"], c["n_samples"], c["seed"])
    return _CACHE["c"]


def test_sampled_state_frequencies_match_the_posteriors(oracle, consistency_samples):
    c = S.consistency_case()
    om = oracle.Model(c["arrays"])
    K = S.CONSISTENCY_COPIES
    worst, n_states = 0.0, 0
    for j in range(0, len(c["reads"]), K):
        read, ls = c["reads"][j], c["lists"][j]
        freq, n = S.emitting_frequencies([consistency_samples[j + i]["rows"] for i in range(K)], len(read), [len(x) for x in ls])
        assert n == K * c["n_samples"]
        o = om.run_with_mapping(read, oracle.Mapping.from_lists(ls))
        for p in range(len(read)):
            m, ins, _, _ = o.to_emit_probs(p + 1)
            for slot, v in enumerate(ls[p]):
                for kind, lp in ((0, m[v]), (1, ins[v])):
                    prob = math.exp(lp)
                    gap = abs(freq[p][slot, kind] - prob)
                    worst = max(worst, gap / S.binomial_bar(prob, n))
                    n_states += 1
                    assert gap <= S.binomial_bar(prob, n), (j, p, slot, kind, freq[p][slot, kind], prob)
    print(f"{n_states} emitting states: the largest gap is {worst:.3f} of its bar")
