"""Alignment records in plain Python (test infrastructure, imported like best_path_ref.py): the restatement that
phmm_run_with_mapping_alignments is held to, written from the text of include/phmm_amd_align.h.  It shares no code with
dbgphmm_amd/model.py.

A path is a sequence of events: per base the emitting state, then the Del states behind it (the entries of the base's
row in the out_path encoding of include/phmm_amd_path.h, up to the padding).  compress() turns rows into the record,
expand() turns a record back into the (node, kind) sequence that dbgphmm_amd.path_states reads off the rows."""
import numpy as np

NONE = 0xFFFFFFFF
INS_BEGIN = 0xFFFFFFFD
INS, DEL, EQ, DIFF = 1, 2, 7, 8
OP_CHARS = {INS: "I", DEL: "D", EQ: "=", DIFF: "X"}


def events(arrays, read, lists, rows):
    """-> [(op, node | None)]: one per event, node for the steps (Match and Del)"""
    emis = arrays.emission.tolist()
    out = []
    for p, x in enumerate(read):
        for c, code in enumerate(np.asarray(rows)[p].tolist()):
            if code == NONE:
                break
            if code == INS_BEGIN:
                out.append((INS, None))
                continue
            node, kind = int(lists[p][code >> 2]), code & 3
            if c == 0 and kind == 0:
                out.append((EQ if emis[node] == x else DIFF, node))
            elif c == 0:
                out.append((INS, None))
            else:
                out.append((DEL, node))
    return out


def compress(arrays, read, lists, rows):
    """-> (cigar, run_node, run_len): cigar the words (len << 4) | op of the maximal runs of equal ops; run_node / run_len
    the maximal runs over the steps in which every node id is the one before plus one"""
    cigar, run_node, run_len = [], [], []
    prev_op, prev_node = None, None
    for op, node in events(arrays, read, lists, rows):
        if op == prev_op:
            cigar[-1] += 1 << 4
        else:
            cigar.append((1 << 4) | op)
        prev_op = op
        if node is not None:
            if prev_node is not None and node == prev_node + 1:
                run_len[-1] += 1
            else:
                run_node.append(node)
                run_len.append(1)
            prev_node = node
    return cigar, run_node, run_len


def expand(cigar, run_node, run_len):
    """-> [(node | None, 'M' | 'I' | 'D' | 'IB')]: =, X and D consume one step each; an I before the first step is
    InsBegin, an I after a step sits on the last step's node"""
    steps = [first + i for first, n in zip(run_node, run_len) for i in range(n)]
    out, k = [], 0
    for w in cigar:
        n, op = w >> 4, w & 15
        for _ in range(n):
            if op == INS:
                out.append((None, "IB") if k == 0 else (steps[k - 1], "I"))
            else:
                out.append((steps[k], "D" if op == DEL else "M"))
                k += 1
    assert k == len(steps), (k, len(steps))
    return out


def cigar_string(cigar):
    return "".join(f"{w >> 4}{OP_CHARS[w & 15]}" for w in cigar)


def op_totals(cigar):
    """-> [=, X, I, D], the order of out_counts"""
    t = {INS: 0, DEL: 0, EQ: 0, DIFF: 0}
    for w in cigar:
        t[w & 15] += w >> 4
    return [t[EQ], t[DIFF], t[INS], t[DEL]]


def check_invariants(cigar, run_node, run_len, length, counts=None):
    """the three invariants of the header, and that the runs are maximal and well formed"""
    eq, diff, ins, dele = op_totals(cigar)
    assert all(w & 15 in OP_CHARS and w >> 4 >= 1 for w in cigar), cigar
    assert all((a & 15) != (b & 15) for a, b in zip(cigar, cigar[1:])), cigar  # maximal runs
    assert len(run_node) == len(run_len) and all(n >= 1 for n in run_len)
    assert all(run_node[i] + run_len[i] != run_node[i + 1] for i in range(len(run_node) - 1)), (run_node, run_len)
    if not cigar:
        assert not run_node
        if counts is not None:
            assert list(counts) == [0, 0, 0, 0]
        return
    assert eq + diff + ins == length, (cigar, length)
    if counts is not None:
        assert [eq, diff, ins, dele] == list(counts), (cigar, list(counts))
    assert sum(run_len) == eq + diff + dele, (run_len, cigar)


def states_of_rows(lists, rows):
    """what dbgphmm_amd.path_states returns, from per-position lists: the row-derived (node, kind) sequence"""
    out = []
    for p, row in enumerate(np.asarray(rows).tolist()):
        for code in row:
            if code == NONE:
                break
            out.append((None, "IB") if code == INS_BEGIN else (int(lists[p][code >> 2]), "MID"[code & 3]))
    return out


def records_of(al, a):
    """alignment a of exported arrays (op_off, ops, run_off, run_node, run_len) -> (cigar, run_node, run_len) as lists"""
    op_off, ops, run_off, rn, rl = al
    o0, o1, r0, r1 = int(op_off[a]), int(op_off[a + 1]), int(run_off[a]), int(run_off[a + 1])
    return ops[o0:o1].tolist(), rn[r0:r1].tolist(), rl[r0:r1].tolist()
