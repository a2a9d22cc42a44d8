"""The restatement of phmm_sample_reads (tests/sample_reads_ref.py) held on its own, without a GPU: its walks follow the
exact law of a tiny model, every decision of every shared fixture stays clear of its boundaries, a history is a walk of
the graph whose emissions are the bases, and the truth of a walk is a path of the forward model."""
import math

import numpy as np

import dbgphmm_amd as D
import sample_reads_ref as G


def test_chi_square_against_the_exact_law():
    arrays, length, kind = G.chi_case()
    law = G.exact_law(arrays, length, kind)
    assert abs(sum(law.values()) - 1.0) <= 1e-12
    outcomes = []
    for i in range(G.CHI_WALKS):
        bases, hist, flags, _ = G.walk(arrays, G.CHI_SEED, i, length, kind)
        outcomes.append((tuple(hist), bases))
    chi, df = G.chi_square(law, outcomes)
    print(f"{len(law)} outcomes, chi-square {chi:.1f} at df {df}, bar {G.chi_bar(df):.1f}")
    assert df >= 50 and chi <= G.chi_bar(df)
    # the case has what the issue asks of it: a branch, a self-loop and a parallel edge on 3 to 5 nodes
    pairs = list(zip(arrays.edge_src.tolist(), arrays.edge_dst.tolist()))
    assert 3 <= arrays.n_nodes <= 5 and any(u == v for u, v in pairs) and len(set(pairs)) < len(pairs)
    assert max(np.bincount(arrays.edge_src)) >= 3


def test_every_fixture_decision_keeps_the_margin():
    worst = math.inf
    for k, f in enumerate(G.fixtures()):
        for w, (_, _, _, margin) in enumerate(G.fixture_walks(k)):
            assert margin >= G.MIN_MARGIN, (f["tag"], w, margin)
            worst = min(worst, margin)
    print(f"{len(G.fixtures())} fixtures: the smallest margin is {worst:.3e}")


def _states(hist):
    return [w for w in hist if w not in (G.END, G.NONE)]


def test_the_shape_of_a_history():
    for k, f in enumerate(G.fixtures()):
        arrays = f["arrays"]
        edges = set(zip(arrays.edge_src.tolist(), arrays.edge_dst.tolist()))
        finite = {e for e, t in zip(zip(arrays.edge_src.tolist(), arrays.edge_dst.tolist()), arrays.trans_logp.tolist())
                  if t > -math.inf}
        for w, (bases, hist, flags, _) in enumerate(G.fixture_walks(k)):
            at = (f["tag"], w)
            states = _states(hist)
            assert hist.count(G.END) == (1 if flags & (G.ENDED | G.DEAD_END) else 0), at
            assert not hist or G.END not in hist[:-1], at
            emitting = [s for s in states if s == G.INS_BEGIN or (s & 3) != G.DEL]
            assert len(emitting) == len(bases) and len(bases) <= f["length"] + 1, at
            n_steps = len(hist) - (1 if f["start_nodes"] else 0)
            if f["kind"] == G.EMIT_COUNT:
                assert len(bases) == f["length"] or flags or (f["start_nodes"] and f["length"] == 1), at
                assert n_steps <= G.state_cap(f["length"]) + 1, at
            else:
                assert n_steps <= f["length"] + 1 and (n_steps == f["length"] or flags), at
            if f["start_nodes"]:
                assert states[0] >> 2 in f["start_nodes"] and states[0] & 3 == G.M, at
            prev = None
            for s in states:
                if s == G.INS_BEGIN:
                    assert prev is None, at  # InsBegin only before the first node state
                    continue
                v, kind = s >> 2, s & 3
                if prev is None:
                    assert kind != G.I and arrays.init_logp[v] > -math.inf, at
                elif kind == G.I:
                    assert v == prev, at  # an Ins stays on its node
                else:
                    assert (prev, v) in edges and (prev, v) in finite, at
                prev = v
            assert set(bases) <= set(b"ACGT"), at


def test_zero_error_reads_are_the_emissions_of_their_match_nodes():
    base = G.model("dbg")
    arrays = D.PHMMArrays(D.PHMMParams.uniform(0.0), base.emission, base.init_logp, base.edge_src, base.edge_dst,
                          base.trans_logp)
    for i in range(40):
        bases, hist, flags, _ = G.walk(arrays, 3, i, 50, G.STATE_COUNT)
        states = _states(hist)
        assert all(s != G.INS_BEGIN and s & 3 == G.M for s in states)
        assert (len(states) == 50 and not flags) or flags == G.DEAD_END  # (a walk may run off the end of a haplotype)
        assert bases == bytes(int(arrays.emission[s >> 2]) for s in states)


def test_the_share_outside_the_forward_model():
    total = outside = 0
    for k, f in enumerate(G.fixtures()):
        for w, (bases, hist, flags, _) in enumerate(G.fixture_walks(k)):
            total += 1
            t = G.truth(f["arrays"], hist, bases)
            if t is None:
                outside += 1
                continue
            lists, rows = t
            value, n_terms, counts = G.score_path(f["arrays"], bases, lists, rows)
            assert math.isfinite(value), (f["tag"], w)
            assert sum(counts[:3]) == len(bases)
    print(f"{outside} of {total} fixture walks lie outside the forward model")
    assert outside <= 0.10 * total
