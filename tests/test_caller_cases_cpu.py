"""No GPU: the table of tests/caller_cases.py covers the ABI, and on_stream always puts the NULL stream back."""
import pytest

import caller_cases as cc


def test_every_prototyped_symbol_has_a_row_or_a_reason():
    in_rows = {s for row in cc.ROWS for s in row.symbols}
    assert not in_rows & set(cc.EXEMPT), sorted(in_rows & set(cc.EXEMPT))
    want = cc.prototyped_symbols()
    have = in_rows | set(cc.EXEMPT)
    assert have == want, (sorted(want - have), sorted(have - want))  # a new entry point needs a row or a reason
    assert all(isinstance(r, str) and len(r.split()) >= 3 for r in cc.EXEMPT.values())
    names = [row.name for row in cc.ROWS]
    assert len(set(names)) == len(names) and all(row.symbols for row in cc.ROWS)


def test_the_rows_the_contract_names_are_there():
    for name in ("run_dense", "run_dense_edges", "run_sparse", "full_prob_sparse_backward", "full_prob_reads",
                 "full_prob_reads_topk", "full_prob_reads_hinted", "full_prob_reads_candidates", "full_prob_reads_copy_nums",
                 "full_prob_reads_copy_num_changes", "generate_mappings", "generate_mappings_carried", "mappings_read_logp",
                 "mappings_read_logp_backward", "mappings_node_freqs", "mappings_map_nodes", "run_with_mapping_edges",
                 "run_with_mapping_states", "run_with_mapping_best_path", "run_with_mapping_sample_paths", "sample_reads",
                 "likelihood_create", "likelihood_score_changes", "likelihood_move", "likelihood_current"):
        assert name in cc.ROW, name


class _FakeLib:
    def __init__(self, log):
        self.log = log

    def phmm_set_stream(self, s):
        self.log.append(("set", s))
        return 0


class _FakeStream:
    def __init__(self, log):
        self.log = log

    def synchronize(self):
        self.log.append(("sync",))


def test_on_stream_restores_the_null_stream_then_drains():
    log = []
    s = _FakeStream(log)
    with cc.on_stream(_FakeLib(log), s) as got:
        assert got is s
        log.append(("body",))
    assert log == [("set", s), ("body",), ("set", None), ("sync",)]


def test_on_stream_restores_when_the_body_raises():
    log = []
    s = _FakeStream(log)
    with pytest.raises(KeyError):
        with cc.on_stream(_FakeLib(log), s):
            raise KeyError("the body failed")
    assert log == [("set", s), ("set", None), ("sync",)]


def test_on_stream_passes_a_raw_handle_through():
    log = []
    with cc.on_stream(_FakeLib(log), 0x1234):
        pass
    assert log == [("set", 0x1234), ("set", None)]
