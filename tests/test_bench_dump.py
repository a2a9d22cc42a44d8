"""CPU: bench.py --dump-outputs' host side -- the fixed sample of a mapping CSR and the size-bounded .npy writer."""
import numpy as np
import pytest

import bench


class _FakeMappings:
    def __init__(self, po, nd, lp):
        self._a = (po, nd, lp)

    def arrays(self):
        return self._a


def _fake(n_pos, seed):
    rng = np.random.default_rng(seed)
    cnt = rng.integers(0, 100, size=n_pos)
    po = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
    nd = rng.integers(0, 1 << 20, size=int(po[-1])).astype(np.uint32)
    lp = -rng.random(int(po[-1])) * 30.0
    return _FakeMappings(po, nd, lp)


@pytest.mark.parametrize("n_pos", [50, 200_000])
def test_mapping_sample_is_fixed_and_holds_the_lists(n_pos):
    mp = _fake(n_pos, seed=n_pos)
    s = bench.mapping_sample(mp)
    again = bench.mapping_sample(_fake(n_pos, seed=n_pos + 1))  # other values, the same read set size
    assert np.array_equal(s["mapping_positions"], again["mapping_positions"])
    po, nd, lp = mp.arrays()
    pos = s["mapping_positions"].astype(np.int64)
    assert pos.size == min(n_pos, 1 << 15) and np.all(np.diff(pos) > 0) and pos[-1] < n_pos
    assert np.array_equal(s["mapping_list_len"], np.diff(po.astype(np.int64))[pos])
    at = 0
    for p in pos:
        lo, hi = int(po[p]), int(po[p + 1])
        k = min(hi - lo, 64)
        assert np.array_equal(s["mapping_nodes"][at:at + k], nd[lo:lo + k])
        assert np.array_equal(s["mapping_logp"][at:at + k], lp[lo:lo + k])
        at += k
    assert s["mapping_nodes"].shape == s["mapping_logp"].shape == (at,)
    assert all(np.all(np.isfinite(a)) for a in s.values())
    assert sum(a.nbytes for a in s.values()) <= 33 << 20


def test_mapping_sample_of_empty_lists():
    s = bench.mapping_sample(_FakeMappings(np.zeros(11, np.uint64), np.zeros(0, np.uint32), np.zeros(0)))
    assert s["mapping_positions"].tolist() == list(range(10)) and not s["mapping_list_len"].any()
    assert s["mapping_nodes"].shape == s["mapping_logp"].shape == (0,)


def test_dump_outputs_writes_float64_and_refuses_oversize(tmp_path):
    bench.dump_outputs(str(tmp_path / "d"), {"a": np.arange(5, dtype=np.uint32), "b": np.ones((2, 3), np.float32)})
    a, b = np.load(tmp_path / "d" / "a.npy"), np.load(tmp_path / "d" / "b.npy")
    assert a.dtype == b.dtype == np.float64 and a.tolist() == [0, 1, 2, 3, 4] and b.shape == (2, 3)
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "big"), {"x": np.zeros(bench.DUMP_LIMIT_BYTES // 8 + 1)})
    assert not (tmp_path / "big").exists()
