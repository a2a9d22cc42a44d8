"""The coverage claims of tests/test_gpu_large_k.py, checked through the oracle without a GPU: the read sets of
large_k_cases hold the classes the GPU tests assume -- switch columns above 255 (past one byte of the uint16 the
library carries them in), switches exactly at n_warmup that are not forced ones, early switches, and cut reads that
stay dense from end to end.  If the PRNG or a dataset changes, this fails, not the coverage."""
import numpy as np
import pytest

import large_k_cases as LK


@pytest.mark.parametrize("name,k", sorted(LK.SETS))
def test_classes_are_populated(oracle, name, k):
    c = LK.classes(oracle, name, k)
    cols, nodes, widths, thr = c["cols"], c["nodes"], c["widths"], c["arrays"].param.warmup_threshold
    lens = np.array([len(r) for r in c["reads"]])
    print(f"\n{name} k={k} N={c['arrays'].n_nodes}: (switch column, nodes inside the ratio, nodes of the first sparse column) "
          + " ".join(f"({a},{b},{w})" for a, b, w in zip(cols, nodes, widths)))
    # every read switches, inside its length and not after n_warmup; none is a forced switch (more than 400 nodes inside
    # the ratio at n_warmup) and no first sparse column fills the 400-slot vector: every read is a parity target
    assert np.all(cols < lens) and np.all(cols <= k) and np.all(cols >= 1)
    assert nodes.max() <= 400 and widths.max() < 400
    # a natural switch is taken at <= warmup_threshold nodes, the one at n_warmup with more
    assert np.all(nodes[cols < k] <= thr) and np.all(nodes[cols == k] > thr)
    sample = LK.oracle_sample(c)
    assert len(sample) <= 10 and len(set(sample.tolist())) == len(sample)
    for cls in ("above_255", "at_warmup", "early"):
        assert len(c[cls]) == 0 or np.intersect1d(sample, c[cls]).size >= 1, cls
    if (name, k) == ("u100n100", 270):
        assert len(c["above_255"]) >= 3 and len(c["early"]) >= 2
        assert len(c["at_warmup"]) >= 2 and np.all((nodes[c["at_warmup"]] >= 201) & (widths[c["at_warmup"]] <= 400))
        assert np.intersect1d(sample, c["at_warmup"]).size >= 2 and np.intersect1d(sample, c["above_255"]).size >= 3
    elif (name, k) == ("u100n100", 300):
        # no read reaches n_warmup here: natural switches only, most of them past column 255
        assert (cols >= 274).sum() >= 10 and cols.max() < 300 and len(c["early"]) >= 2
    elif (name, k) == ("u20n200", 300):
        # late switches of short heads with wide first sparse columns
        assert cols.max() <= 200 and (widths[cols >= 80] > 300).sum() >= 2
    else:
        # k longer than the reads: they still switch, past column 255
        assert lens.max() < k and cols.min() > 255


def test_cut_reads_are_dense_from_end_to_end(oracle):
    c = LK.classes(oracle, "u100n100", 270)
    k, om = 270, oracle.Model(c["arrays"])
    reads, names = LK.seam_reads(c)
    assert [len(r) for r in reads[:5]] == [k - 1, k, k + 1, k + 2, k + 3] and len(reads[5]) == 150 and len(reads[6]) > 255
    cols, _, _ = LK.switches(oracle, om, reads)
    print("\n" + ", ".join(f"{n}: {c}" for n, c in zip(names, cols)))
    # n_warmup - 1 and n_warmup bases end inside the dense head; from n_warmup + 1 on the switch is at n_warmup
    assert cols.tolist()[:5] == [k - 1, k, k, k, k]
    for r in reads[:2] + reads[5:]:
        assert LK.dense_end_to_end(oracle, om, r)
    assert cols[5] == 150 and cols[6] == len(reads[6])
    # the 1100-set's cut read (280 bases) switches nowhere either: its column would be past its end
    c2 = LK.classes(oracle, "u100n100", 1100)
    assert c2["cols"][0] > 280 and LK.dense_end_to_end(oracle, oracle.Model(c2["arrays"]), c2["reads"][0][:280])


def test_a_600_base_read_pins_the_backward_sparse_tables(oracle):
    """fixed mode at n_warmup = 300, n_active_nodes = 200: among the first eight reads cut to 600 bases there is one
    whose backward_sparse tables do not depend on the oracle's tie rule, and reads that do (what the GPU test assumes
    when it holds every column of that read at 1e-8)"""
    import dbgphmm_amd as D
    c = LK.classes(oracle, "u100n100", 300)
    arrays = D.vectorised_to_phmm(c["sg"], c["arrays"].param.with_(n_active_nodes=200), 1)
    pinned, stable = LK.tie_stable_cut(oracle, oracle.Model(arrays), c["reads"][:8], 600)
    print(f"\npinned {pinned}, {stable}")
    assert pinned is not None and not all(stable)
