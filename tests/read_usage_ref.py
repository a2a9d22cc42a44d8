"""A numpy restatement of phmm_run_with_mapping_read_usage's reduction (include/phmm_amd_usage.h): from the per-entry
values of the states call to the sparse read-by-key matrix.  Every sum is math.fsum, the exactly rounded sum, so the
restatement has no order and at most half an ulp of error of its own.  No GPU, no library."""
import math

import numpy as np

NONE = 0xFFFFFFFF


def key_map(n_nodes, groups):
    """-> (key_of[N] with NONE for a node in no group, K); groups = (group_off, group_nodes) or None"""
    if groups is None:
        return np.arange(n_nodes, dtype=np.uint32), n_nodes
    g_off, g_nodes = np.asarray(groups[0], dtype=np.int64), np.asarray(groups[1], dtype=np.int64)
    key_of = np.full(n_nodes, NONE, dtype=np.uint32)
    for g in range(g_off.size - 1):
        for v in g_nodes[g_off[g]:g_off[g + 1]]:
            assert key_of[v] == NONE
            key_of[v] = g
    return key_of, g_off.size - 1


def read_usage_ref(read_off, pos_off, nodes, state_logp, n_nodes, groups=None):
    """read_off[R + 1] (bases), pos_off[total_bases + 1], nodes[entries], state_logp[entries, 3] (natural logs, -inf
    allowed) -> (row_off[R + 1] uint64, keys uint32, usage[., 3], totals[K, 3], terms[.]): per read the distinct keys
    among its entries in ascending order; usage = fsum of exp(state_logp) over the read's entries with the key, by
    state; totals = fsum of the rows by key; terms = how many entries each row entry sums"""
    read_off, pos_off = np.asarray(read_off, dtype=np.int64), np.asarray(pos_off, dtype=np.int64)
    nodes = np.asarray(nodes, dtype=np.int64)
    key_of, K = key_map(n_nodes, groups)
    with np.errstate(under="ignore"):
        prob = np.exp(np.asarray(state_logp, dtype=np.float64).reshape(-1, 3))  # exp(-inf) = 0 exactly
    row_off, keys, usage, terms = [0], [], [], []
    cols = [[[], [], []] for _ in range(K)]
    for r in range(read_off.size - 1):
        a0, a1 = int(pos_off[read_off[r]]), int(pos_off[read_off[r + 1]])
        k = key_of[nodes[a0:a1]]
        order = np.argsort(k, kind="stable")
        order = order[k[order] != NONE]
        uniq, first = np.unique(k[order], return_index=True)
        for key, sel in zip(uniq.tolist(), np.split(a0 + order, first[1:])):
            row = [math.fsum(prob[sel, s].tolist()) for s in range(3)]
            keys.append(key)
            usage.append(row)
            terms.append(sel.size)
            for s in range(3):
                cols[key][s].append(row[s])
        row_off.append(len(keys))
    totals = np.array([[math.fsum(c[s]) for s in range(3)] for c in cols], dtype=np.float64).reshape(K, 3)
    return (np.array(row_off, dtype=np.uint64), np.array(keys, dtype=np.uint32),
            np.array(usage, dtype=np.float64).reshape(-1, 3), totals, np.array(terms, dtype=np.int64))
