"""Prefix sharing of the dense head ("Prefix sharing"): the first J dense forward columns of the
main adaptive plan are computed once per distinct prefix on 4^J virtual reads.  Every case runs the same calls with
PHMM_SHARE_PREFIX=0 and with sharing and requires the same bits -- mapping lists, forward and backward ln P per read,
node usage, the dense columns and flags of last_call_info -- and the J that phmm_last_call_prefix_share reports.

Each run is a fresh child process (this file, run as a script): a process that has made the unshared call holds the
reads' own columns 0 .. J-2 in its workspace, exactly where a shared call that read the wrong table would look.  One
child makes all calls of its read set -- generate_mappings cold, again on the same ReadCollection (hinted grouping),
and to_full_prob_reads without mappings -- and the tests share its arrays.

Read sets: cfg1m (bench.WORKLOADS, N about 5 800, dense for 11-15 columns) cut to 200 reads, 4 groups at W = 64."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("po", "nd", "lp", "lf", "lb", "nf", "cols", "flags")
DECLINE_J = 3
DECLINE_SETS = ("short", "nbase", "tiny", "nwarm")


# ---------------------------------------------------------------- the child process
def _cfg1m(n_warmup=None):
    import bench
    import dbgphmm_amd as D
    arrays, reads, w = bench.build_workload("cfg1m", 0)
    if n_warmup is not None:
        param = D.PHMMParams.uniform(w["p"]).with_(n_warmup=n_warmup)
        arrays = D.vectorised_to_phmm(bench.cfg_seq_graph("cfg1m"), param, 1)
    return arrays, [bytes(r) for r in reads]


def read_set(name):
    """-> (arrays, reads); every set is deterministic"""
    import dbgphmm_amd as D
    if name == "cfg1m":
        arrays, reads = _cfg1m()
        return arrays, reads[:200]
    if name == "same4":  # many lanes on one virtual lane
        arrays, reads = _cfg1m()
        return arrays, [reads[0][:4] + r[4:] for r in reads[:70]]
    if name == "pairs16":  # J = 2: every virtual lane used
        arrays, reads = _cfg1m()
        pairs = [bytes([a, b]) for a in b"ACGT" for b in b"ACGT"]
        return arrays, [pairs[j % 16] + r[2:] for j, r in enumerate(reads[:70])]
    if name == "auto_short":  # the planner's own J (3 at 4 groups) with reads of 2 and 4 bases in the set
        arrays, reads = _cfg1m()
        return arrays, reads[:100] + [reads[200][:2]] + reads[100:200] + [reads[201][:4]]
    if name == "short":  # one read of J + 1 bases
        arrays, reads = _cfg1m()
        return arrays, reads[:100] + [reads[100][: DECLINE_J + 1]]
    if name == "nbase":  # a base the model does not emit among the first J
        arrays, reads = _cfg1m()
        return arrays, reads[:100] + [reads[100][:2] + b"N" + reads[100][3:]]
    if name == "nwarm":  # the forced switch falls on launch J
        arrays, reads = _cfg1m(n_warmup=DECLINE_J + 1)
        return arrays, reads[:100]
    if name == "tiny":  # N <= warmup_threshold: every read leaves the warm-up at position 1
        sg = D.dbg_from_haplotypes([D.random_genome(150, seed=11)], 16)
        arrays = D.vectorised_to_phmm(sg, D.PHMMParams.uniform(0.001).with_(n_warmup=16), 1)
        assert arrays.n_nodes <= 200
        # (reads of J + 2 bases or more: the length rule must not be what declines)
        return arrays, [bytes(r) for r in D.sample_reads(arrays, 10 ** 9, 60, seed=7, max_reads=120) if len(r) >= 8][:100]
    raise KeyError(name)


def _calls(arrays, reads):
    import dbgphmm_amd as D
    from dbgphmm_amd import _ffi
    out = {}
    gm, rc = D.PHMMModel(arrays), D.ReadCollection(reads)
    for tag in ("cold", "hinted"):  # the second call groups the reads by the first one's dense columns
        mp, nf = gm.generate_mappings(rc, None, True)
        j, lanes = _ffi.last_call_prefix_share()
        cells = _ffi.last_call_stats(_ffi.PHMM_STATS_DENSE_FWD)[2]
        cols, flags = rc.last_call_info()
        po, nd, lp = mp.arrays()
        vals = (po, nd, lp, mp.read_logp()[1], mp.read_logp_backward()[1], nf, cols, flags)
        out.update({f"{tag}_{k}": np.array(v) for k, v in zip(KEYS, vals)})
        out[f"{tag}_share"] = np.array([j, lanes, cells], dtype=np.int64)
    rc2 = D.ReadCollection(reads)  # forward only: the adaptive forward without a sink
    _, lf = gm.to_full_prob_reads(rc2, None, True)
    cols, flags = rc2.last_call_info()
    j, lanes = _ffi.last_call_prefix_share()
    out.update(fwd_lf=np.array(lf), fwd_cols=np.array(cols), fwd_flags=np.array(flags),
               fwd_share=np.array([j, lanes, _ffi.last_call_stats(_ffi.PHMM_STATS_DENSE_FWD)[2]], dtype=np.int64))
    out["n_nodes"] = np.array([arrays.n_nodes, len(reads), min(map(len, reads))], dtype=np.int64)
    return out


def _child(names, path):
    out = {}
    for name in names.split(","):
        arrays, reads = read_set(name)
        out.update({f"{name}.{k}": v for k, v in _calls(arrays, reads).items()})
    np.savez(path, **out)


if __name__ == "__main__":
    for p in (HERE, ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)
    _child(sys.argv[1], sys.argv[2])
    sys.exit(0)


# ---------------------------------------------------------------- the tests
pytestmark = pytest.mark.gpu
_cache = {}


def run(tmp_path_factory, names, share, **env):
    """the arrays of one child: read sets `names` (comma-separated) under PHMM_SHARE_PREFIX=share and env"""
    key = (names, share, tuple(sorted(env.items())))
    if key not in _cache:
        e = dict(os.environ, PHMM_DENSE_W="64", **env)
        e.pop("PHMM_SHARE_PREFIX", None)
        if share is not None:  # (None: the planner's choice)
            e["PHMM_SHARE_PREFIX"] = str(share)
        path = str(tmp_path_factory.mktemp("share") / "out.npz")
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), names, path]
        r = subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-4000:]
        with np.load(path) as z:
            _cache[key] = {k: z[k] for k in z.files}
    return _cache[key]


def same(on, off, name, tags=("cold", "hinted")):
    for tag in tags:
        for k in KEYS:
            assert np.array_equal(on[f"{name}.{tag}_{k}"], off[f"{name}.{tag}_{k}"]), (name, tag, k)
    for k in ("lf", "cols", "flags"):
        assert np.array_equal(on[f"{name}.fwd_{k}"], off[f"{name}.fwd_{k}"]), (name, "fwd", k)


def shared_j(z, name, tag):
    return tuple(int(x) for x in z[f"{name}.{tag}_share"][:2])


def check_cells(on, off, name, J):
    """phmm_last_call_stats(0): the virtual plan's cells come in, J columns of every read go"""
    n, r, _ = (int(x) for x in on[f"{name}.n_nodes"])
    for tag in ("cold", "hinted", "fwd"):
        if np.any(on[f"{name}.{tag}_flags"]):
            continue  # (a read that left the main plan is not in its count)
        assert int(off[f"{name}.{tag}_share"][2]) - int(on[f"{name}.{tag}_share"][2]) == (r - 4 ** J) * J * n, (name, tag)


@pytest.mark.parametrize("J", [2, 3, 4])
def test_lane_mapping_across_groups(gpu_lib, tmp_path_factory, J):
    """4 read groups, forced J: at J = 4 the lanes of one group map to all four virtual groups"""
    on, off = run(tmp_path_factory, "cfg1m", J), run(tmp_path_factory, "cfg1m", 0)
    assert int(on["cfg1m.n_nodes"][1]) == 200 and int(on["cfg1m.n_nodes"][2]) >= 8
    assert shared_j(on, "cfg1m", "cold") == (J, 4 ** J) and shared_j(off, "cfg1m", "cold") == (0, 0)
    same(on, off, "cfg1m", tags=("cold",))
    assert int(on["cfg1m.cold_cols"].min()) >= J  # nobody left the warm-up inside the shared columns
    check_cells(on, off, "cfg1m", J)


@pytest.mark.parametrize("J", [2, 4])
def test_hinted_grouping(gpu_lib, tmp_path_factory, J):
    """the second call on the same ReadCollection groups by the hints: against its unshared twin and the cold call"""
    on, off = run(tmp_path_factory, "cfg1m", J), run(tmp_path_factory, "cfg1m", 0)
    assert shared_j(on, "cfg1m", "hinted") == (J, 4 ** J)
    same(on, off, "cfg1m", tags=("hinted",))
    for k in KEYS:
        assert np.array_equal(on[f"cfg1m.hinted_{k}"], on[f"cfg1m.cold_{k}"]), k


@pytest.mark.parametrize("env", [{"PHMM_CHUNK_GROUPS": "2"},
                                 {"PHMM_WORKERS": "2", "PHMM_PIPELINE_MIN_GROUPS": "1", "PHMM_CHUNK_GROUPS": "2"}],
                         ids=["chunks", "workers"])
def test_chunk_seams_and_workers(gpu_lib, tmp_path_factory, env):
    """two chunks of two groups, on one stream and on two worker threads: all read the one virtual plan"""
    on, off = run(tmp_path_factory, "cfg1m", 4, **env), run(tmp_path_factory, "cfg1m", 0, **env)
    assert shared_j(on, "cfg1m", "cold") == (4, 256) and shared_j(on, "cfg1m", "hinted") == (4, 256)
    same(on, off, "cfg1m")
    same(on, run(tmp_path_factory, "cfg1m", 0), "cfg1m", tags=("cold",))


@pytest.mark.parametrize("name,J", [("same4", 4), ("pairs16", 2)])
def test_duplicate_prefixes(gpu_lib, tmp_path_factory, name, J):
    """70 reads on one virtual lane of 256, and 70 reads over all 16 virtual lanes of J = 2 (an incomplete group)"""
    on, off = run(tmp_path_factory, name, J), run(tmp_path_factory, name, 0)
    assert shared_j(on, name, "cold") == (J, 4 ** J)
    same(on, off, name)
    check_cells(on, off, name, J)


def test_forward_only(gpu_lib, tmp_path_factory):
    """to_full_prob_reads without mappings: the adaptive forward without a sink shares too"""
    on, off = run(tmp_path_factory, "cfg1m", 4), run(tmp_path_factory, "cfg1m", 0)
    assert shared_j(on, "cfg1m", "fwd") == (4, 256) and shared_j(off, "cfg1m", "fwd") == (0, 0)
    for k in ("lf", "cols", "flags"):
        assert np.array_equal(on[f"cfg1m.fwd_{k}"], off[f"cfg1m.fwd_{k}"]), k
    assert np.array_equal(on["cfg1m.fwd_lf"], on["cfg1m.cold_lf"])


def test_planner_sets_short_reads_aside(gpu_lib, tmp_path_factory):
    """PHMM_SHARE_PREFIX unset: the planner takes J = 3 for 4 groups; the two reads of less than J + 2 bases run in an
    unshared plan of their own and the other 200 share (a forced J declines on such a set: test_declines[short])"""
    on, off = run(tmp_path_factory, "auto_short", None), run(tmp_path_factory, "auto_short", 0)
    assert int(on["auto_short.n_nodes"][1]) == 202 and int(on["auto_short.n_nodes"][2]) == 2
    for tag in ("cold", "hinted", "fwd"):
        assert shared_j(on, "auto_short", tag) == (3, 64) and shared_j(off, "auto_short", tag) == (0, 0)
    same(on, off, "auto_short")


@pytest.mark.parametrize("name", DECLINE_SETS)
def test_declines(gpu_lib, tmp_path_factory, name):
    """a read of J + 1 bases; a third base N; a graph where every read switches at position 1; n_warmup = J + 1:
    the plan runs unshared, the getter says 0"""
    names = ",".join(DECLINE_SETS)
    on, off = run(tmp_path_factory, names, DECLINE_J), run(tmp_path_factory, names, 0)
    for tag in ("cold", "hinted", "fwd"):
        assert shared_j(on, name, tag) == (0, 0), (name, tag)
    same(on, off, name)
    if name == "tiny":
        assert int(on["tiny.cold_cols"].max()) == 1 and int(on["tiny.n_nodes"][0]) <= 200
    if name == "short":
        assert int(on["short.n_nodes"][2]) == DECLINE_J + 1
