"""Read sets for the regime n_warmup = k >= 250 (the reference grows k from 40 to thousands and runs generate_mappings
with n_warmup = k at every step: multi_dbg.rs:1394-1409, posterior.rs:735-810): the first reads of the tandem-repeat
datasets of repeat_cases at large k, and the reads of each set picked by PROPERTY through the oracle -- where the
adaptive forward (forward.rs:107-137) leaves its dense head.

switch column of a read = number of dense forward tables of the oracle's FWD_SPARSE_RATIO run (len(read) when the read
never switches); nodes at the switch = number of nodes inside the score ratio in the last dense column -- the number
that decides: above warmup_threshold (200) the next column stays dense while it is inside the warm-up, above 400 at
n_warmup the switch is a forced one (outside the parity domain).

tests/test_large_k_cases_cpu.py asserts that every class is populated as tests/test_gpu_large_k.py assumes.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from repeat_cases import dataset

# (dataset, k) -> number of first reads used
SETS = {("u100n100", 270): 12, ("u100n100", 300): 24, ("u20n200", 300): 24, ("u100n100", 1100): 4}

MARGIN = 1e-6  # nats around the ratio cut inside which a node may fall on either side


def ratio_count(table, ratio, margin=MARGIN):
    """Nodes of one forward table (m, i, d, scalars) inside the score ratio (table.rs:134-149: best - value < ratio over
    m + i + d) -> (count, count of those more than `margin` inside the cut, count with those up to `margin` outside)."""
    m, i, d, _ = table
    with np.errstate(divide="ignore"):
        v = np.logaddexp(np.logaddexp(m, i), d)
    gap = v.max() - v
    return int((gap < ratio).sum()), int((gap < ratio - margin).sum()), int((gap < ratio + margin).sum())


def switch_of(oracle, om, read):
    """-> (switch column, nodes at the switch, nodes of the first sparse column: the former with their children); zeros
    for a read that never switches.  Only the first n_warmup + 1 bases decide (column n_warmup is never dense)."""
    head = read[:om.param.n_warmup + 1]
    f = om.forward(head, oracle.FWD_SPARSE_RATIO)
    col = next((i for i in range(len(head)) if not f.is_dense(i)), len(head))
    if col == len(head):
        assert len(head) == len(read)
        return col, 0, 0
    return col, ratio_count(f.table(col - 1), om.param.active_node_max_ratio)[0], len(f.nodes(col, 0))


def switches(oracle, om, reads, n_threads=16):
    """switch_of for every read (the oracle's entry points keep their state per thread) -> (columns, nodes, widths)"""
    with ThreadPoolExecutor(n_threads) as ex:
        out = list(ex.map(lambda r: switch_of(oracle, om, r), reads))
    return tuple(np.array(x, dtype=np.int64) for x in zip(*out))


def dispute(oracle, om, read, col_a, col_b):
    """Two switch columns of one read that differ: at the earlier one, c, one side left the dense head and the other
    did not, both from the same column c - 1.  That is a matter of rounding only when the count of nodes inside the ratio
    there crosses warmup_threshold with the nodes within MARGIN of the cut (best - active_node_max_ratio) -> dict with
    `allowed` and the counts (exact, without / with the nodes in the margin)."""
    c, p = int(min(col_a, col_b)), om.param
    if not 0 < c < p.n_warmup:  # column 0 is always dense, column n_warmup never
        return dict(column=c, allowed=False)
    f = om.forward(read[:c], oracle.FWD_SPARSE_RATIO)
    assert all(f.is_dense(i) for i in range(c))
    count, inside, outside = ratio_count(f.table(c - 1), p.active_node_max_ratio)
    return dict(column=c, count=count, inside=inside, outside=outside, allowed=inside <= p.warmup_threshold < outside)


# tie rules of the oracle's test hook (orc_set_tie_rule) that bucket near-equal values and keep the order of equal ones
BUCKET_RULES = ((1e-9, 0), (1e-9, 2), (1e-6, 0), (1e-6, 2))


def _sparse_backward_columns(oracle, om, read):
    """the sparse columns of backward_sparse (backward.rs:146-185) of one read, each table as (stored nodes, values)"""
    t = om.backward(read, oracle.BWD_SPARSE)
    out = []
    for i in range(len(read)):
        if t.is_dense(i):
            break
        out.append([(np.flatnonzero(np.isfinite(x)), x[np.isfinite(x)]) for x in t.table(i)[:3]])
    return out


def tie_stable_cut(oracle, om, reads, length, tol=1e-8, n_threads=16):
    """backward_sparse takes every sparse column from the n_active_nodes best nodes of the next one.  On a repeat that
    cut meets equal values all the time (the two haplotype copies of a k-mer).  Values equal to the last bit are kept in
    storage order, by the reference, the oracle and the kernels alike; values that differ by rounding noise only are
    not pinned by the reference at all, and then neither are the tables behind them.  -> index of
    the first read whose first `length` bases give the oracle the same sparse columns (same elements, values within
    `tol`) under its own order and under every rule of BUCKET_RULES: a read on which no decision hangs on noise."""
    import ctypes as C
    lib = oracle.lib()
    lib.orc_set_tie_rule.argtypes = [C.c_double, C.c_int]
    cuts = [r[:length] for r in reads]

    def run():
        with ThreadPoolExecutor(n_threads) as ex:
            return list(ex.map(lambda r: _sparse_backward_columns(oracle, om, r), cuts))

    def same(a, b):
        return len(a) == len(b) and all(np.array_equal(x[0], y[0]) and np.all(np.abs(x[1] - y[1]) <= tol)
                                        for ca, cb in zip(a, b) for x, y in zip(ca, cb))
    base = run()
    stable = [len(r) == length for r in cuts]
    for eps, mode in BUCKET_RULES:
        lib.orc_set_tie_rule(eps, mode)
        try:
            alt = run()
        finally:
            lib.orc_set_tie_rule(0.0, 0)
        stable = [s and same(a, b) for s, a, b in zip(stable, base, alt)]
    return next((j for j, s in enumerate(stable) if s), None), stable


def dense_end_to_end(oracle, om, read):
    f = om.forward(read, oracle.FWD_SPARSE_RATIO)
    return all(f.is_dense(i) for i in range(len(read)))


_CACHE = {}


def classes(oracle, name, k):
    """The read set (name, k) and its classes -> dict: arrays, sg, reads, cols, nodes, widths (per read, from the oracle) and
    index arrays above_255 (switch column > 255), at_warmup (== n_warmup), early (< 120), rest."""
    key = (name, k)
    if key not in _CACHE:
        arrays, reads, sg, _ = dataset(name, k, max_reads=SETS[key])
        assert arrays.param.n_warmup == k
        cols, nodes, widths = switches(oracle, oracle.Model(arrays), reads)
        _CACHE[key] = dict(arrays=arrays, sg=sg, reads=reads, cols=cols, nodes=nodes, widths=widths,
                           above_255=np.flatnonzero((cols > 255) & (cols < k)), at_warmup=np.flatnonzero(cols == k),
                           early=np.flatnonzero(cols < 120), rest=np.flatnonzero((cols >= 120) & (cols <= 255)))
    return _CACHE[key]


def oracle_sample(c, limit=10):
    """At most `limit` reads that cover every class of the set: the classes in turn, latest switch first in the late
    classes, earliest first in the early one."""
    order = [c["above_255"][np.argsort(-c["cols"][c["above_255"]], kind="stable")],
             c["at_warmup"], c["early"][np.argsort(c["cols"][c["early"]], kind="stable")],
             c["rest"][np.argsort(-c["cols"][c["rest"]], kind="stable")]]
    pick, depth = [], 0
    while len(pick) < min(limit, len(c["reads"])):
        for cls in order:
            if depth < len(cls) and len(pick) < limit:
                pick.append(int(cls[depth]))
        depth += 1
    return np.array(sorted(pick), dtype=np.int64)


def seam_reads(c):
    """-> (reads, names): a read that switches at n_warmup cut to n_warmup - 1 ... n_warmup + 3 bases; the latest
    natural switch of the set cut to 150 bases and to (its switch column - 1) bases: both dense from end to end."""
    k, reads = c["arrays"].param.n_warmup, c["reads"]
    at = int(c["at_warmup"][0])
    late = int(max(c["above_255"], key=lambda i: c["cols"][i]))
    out = [(reads[at][:k + d], f"read {at} cut to n_warmup{d:+d}") for d in (-1, 0, 1, 2, 3)]
    out += [(reads[late][:150], f"read {late} cut to 150"),
            (reads[late][:int(c["cols"][late]) - 1], f"read {late} cut to its switch column - 1")]
    return [r for r, _ in out], [n for _, n in out]
