"""GPU: bench.py's result line and --dump-outputs.  What a plain run dumps is what the timed call computes for the
same inputs in another process; --full adds the CPU baseline and the extra measurements of the mapping step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import dbgphmm_amd as D

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def load_dump(path):
    got = {p[:-4]: np.load(os.path.join(path, p)) for p in os.listdir(path)}
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    return got


def test_plain_run_dumps_the_mapping_step(gpu_lib, tmp_path):
    import bench
    j = run_bench("--workload", "cfg1m", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert j["steps"] == 3 and j["warmup"] == 1 and j["ms_per_step"] > 0 and j["dtype"] == "f64"
    assert "cpu_baseline" not in j and "cold_hint_ms" not in j["config"]
    got = load_dump(str(tmp_path))
    assert set(got) == {"read_logp", "node_freq", "mapping_positions", "mapping_list_len", "mapping_nodes", "mapping_logp"}
    assert all(np.all(np.isfinite(a)) for a in got.values())
    arrays, reads, _ = bench.build_workload("cfg1m")
    mp, nf = D.PHMMModel(arrays).generate_mappings(D.ReadCollection(reads), None, True)
    _, lp = mp.read_logp()
    assert np.max(np.abs(got["read_logp"] - lp)) < 1e-9
    assert np.max(np.abs(got["node_freq"] - nf)) < 1e-9
    ref = bench.mapping_sample(mp)
    assert np.array_equal(got["mapping_positions"], ref["mapping_positions"])
    assert np.array_equal(got["mapping_list_len"], ref["mapping_list_len"])
    assert got["mapping_nodes"].shape == ref["mapping_nodes"].shape
    np.testing.assert_allclose(got["mapping_logp"], ref["mapping_logp"], rtol=0, atol=1e-9)
    # another grouping of the reads may swap two entries of one list whose values are equal (tests/helpers.same_mappings)
    take = np.minimum(ref["mapping_list_len"], 64).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(take)])
    for i in np.flatnonzero(got["mapping_nodes"] != ref["mapping_nodes"]):
        row = np.searchsorted(start, i, side="right") - 1
        nodes, logp = ref["mapping_nodes"][start[row]:start[row + 1]], ref["mapping_logp"][start[row]:start[row + 1]]
        partner = np.flatnonzero(nodes == got["mapping_nodes"][i])
        assert partner.size == 1 and abs(logp[partner[0]] - ref["mapping_logp"][i]) < 1e-9


def test_plain_run_dumps_the_dense_step(gpu_lib, tmp_path):
    import bench
    run_bench("--workload", "cfg1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path))
    got = load_dump(str(tmp_path))
    assert set(got) == {"read_logp", "read_logp_backward", "node_freq"}
    assert all(np.all(np.isfinite(a)) for a in got.values())
    arrays, reads, _ = bench.build_workload("cfg1")
    lf, lb, nf = D.PHMMModel(arrays).run_dense(D.ReadCollection(reads))
    for name, want in (("read_logp", lf), ("read_logp_backward", lb), ("node_freq", nf)):
        assert np.max(np.abs(got[name] - want)) < 1e-9, name


def test_candidates_dump(gpu_lib, tmp_path):
    run_bench("--workload", "cfg1m", "--mode", "candidates", "--candidates", "6", "--steps", "2", "--warmup", "1",
              "--dump-outputs", str(tmp_path))
    got = load_dump(str(tmp_path))
    tot, per_read = got["candidate_logp_total"], got["candidate_read_logp"]
    assert tot.shape == (6,) and per_read.shape == (6, got["candidate_read_index"].shape[0])
    assert np.isfinite(tot[0])  # candidate 0: the mapping model's own copy numbers
    np.testing.assert_allclose(per_read.sum(axis=1), tot, rtol=1e-9)  # the total is the sum of logs over the reads


def test_full_run_keeps_the_extra_measurements(gpu_lib):
    j = run_bench("--workload", "cfg1m", "--steps", "1", "--warmup", "1", "--full")
    assert j["steps"] == 1 and j["ms_per_step"] > 0
    assert j["cpu_baseline"]["max_abs_dlogp"] < 1e-6 and j["cpu_baseline"]["value"] > 0
    assert j["config"]["cold_hint_ms"] > 0 and "frontier" in j["config"] and j["config"]["hinted_forward_ms"] > 0
