"""A numpy restatement of phmm_run_with_mapping_pileup's reduction (include/phmm_amd_pileup.h): from the per-entry values
of the states call and the read bases to the sparse read-by-(node, base) matrix and the per-node totals.  Every sum is
math.fsum, the exactly rounded sum, so the restatement has no order and at most half an ulp of error of its own.
No GPU, no library."""
import math

import numpy as np

CODE = np.full(256, -1, dtype=np.int64)
CODE[[ord("A"), ord("C"), ord("G"), ord("T")]] = np.arange(4)


def entry_positions(pos_off, a0, a1):
    """the position of the entries a0 .. a1-1: the last g with pos_off[g] <= a < pos_off[g + 1] (empty lists passed over)"""
    return np.searchsorted(np.asarray(pos_off, dtype=np.int64), np.arange(a0, a1, dtype=np.int64), side="right") - 1


def pileup_ref(read_off, bases, pos_off, nodes, state_logp, n_nodes):
    """read_off[R + 1] (positions), bases[total positions] (ASCII), pos_off[total positions + 1], nodes[entries],
    state_logp[entries, 3] (natural logs, -inf allowed) -> (row_off[R + 1] uint64, keys uint32, usage[., 3],
    totals[N, 9], terms[.]): per read the distinct keys 4 * node + base code among its entries in ascending order;
    usage = fsum of exp(state_logp) over the read's entries with the key, by state; totals = per node the fsum of the
    rows' Match values by base (0-3), Ins values by base (4-7) and Del values (8); terms = how many entries each row
    entry sums"""
    read_off, pos_off = np.asarray(read_off, dtype=np.int64), np.asarray(pos_off, dtype=np.int64)
    nodes = np.asarray(nodes, dtype=np.int64)
    bases = np.frombuffer(bases, dtype=np.uint8) if isinstance(bases, (bytes, bytearray)) else np.asarray(bases, dtype=np.uint8)
    with np.errstate(under="ignore"):
        prob = np.exp(np.asarray(state_logp, dtype=np.float64).reshape(-1, 3))  # exp(-inf) = 0 exactly
    row_off, keys, usage, terms = [0], [], [], []
    cols = [[[] for _ in range(9)] for _ in range(n_nodes)]
    for r in range(read_off.size - 1):
        a0, a1 = int(pos_off[read_off[r]]), int(pos_off[read_off[r + 1]])
        g = entry_positions(pos_off, a0, a1)
        assert np.all((g >= read_off[r]) & (g < read_off[r + 1]))
        c = CODE[bases[g]]
        assert np.all(c >= 0), "a read byte that is none of A C G T"
        k = 4 * nodes[a0:a1] + c
        order = np.argsort(k, kind="stable")
        uniq, first = np.unique(k[order], return_index=True)
        for key, sel in zip(uniq.tolist(), np.split(a0 + order, first[1:])):
            row = [math.fsum(prob[sel, s].tolist()) for s in range(3)]
            keys.append(key)
            usage.append(row)
            terms.append(sel.size)
            v, b = divmod(key, 4)
            cols[v][b].append(row[0])
            cols[v][4 + b].append(row[1])
            cols[v][8].append(row[2])
        row_off.append(len(keys))
    totals = np.array([[math.fsum(c) for c in node] for node in cols], dtype=np.float64).reshape(n_nodes, 9)
    return (np.array(row_off, dtype=np.uint64), np.array(keys, dtype=np.uint32),
            np.array(usage, dtype=np.float64).reshape(-1, 3), totals, np.array(terms, dtype=np.int64))
