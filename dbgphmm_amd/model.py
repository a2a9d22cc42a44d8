"""Host-side mirror of the reference's `PHMMModel` call surface over the C ABI.

Method names, argument meaning and error behaviour follow the reference
(`impl PHMMModel`, /root/reference/src/hmmv2/{forward,backward,freq,hint}.rs) so that the
parity tests read like the reference's own tests.  All compute happens in
libphmm_amd.so (HIP, gfx950); this module only marshals arrays.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _ffi
from .graph import PHMMArrays
from .params import PHMMParams


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(C.c_void_p)
    # torch tensor (device or host output buffer)
    return C.c_void_p(a.data_ptr())


class ReadCollection:
    """ReadCollection<S> (src/common/collection.rs:38-83): concatenated bases + offsets."""

    def __init__(self, reads: Sequence[bytes]):
        self.reads = [bytes(r) for r in reads]
        self.offsets = np.zeros(len(self.reads) + 1, dtype=np.uint64)
        self.offsets[1:] = np.cumsum([len(r) for r in self.reads])
        self.bases = np.frombuffer(b"".join(self.reads), dtype=np.uint8)
        if self.bases.shape[0] == 0:
            self.bases = np.zeros(1, dtype=np.uint8)
        h = C.c_void_p()
        _ffi.check(_ffi.lib().phmm_reads_create(_ptr(self.bases), _ptr(self.offsets), len(self.reads), C.byref(h)))
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            _ffi.lib().phmm_reads_destroy(self._h)
            self._h = None

    def __len__(self) -> int:
        return len(self.reads)

    def total_bases(self) -> int:
        return int(self.offsets[-1])

    def last_call_info(self) -> Tuple[np.ndarray, np.ndarray]:
        """(dense warm-up columns[R], PHMM_READ_* flags[R]) of the most recent adaptive-sparse call."""
        cols = np.empty(len(self.reads), dtype=np.uint16)
        flags = np.empty(len(self.reads), dtype=np.uint32)
        _ffi.check(_ffi.lib().phmm_reads_last_call_info(self._h, _ptr(cols), _ptr(flags)))
        return cols, flags


class Mappings:
    """Mappings (src/hmmv2/hint.rs:150-152) over a ReadCollection: 3-level CSR."""

    def __init__(self, handle, reads: ReadCollection):
        self._h = handle
        self.reads = reads
        self._cache = None

    @staticmethod
    def from_arrays(reads: ReadCollection, pos_off: np.ndarray, nodes: np.ndarray,
                    logp: Optional[np.ndarray] = None) -> "Mappings":
        po = np.ascontiguousarray(pos_off, dtype=np.uint64)
        nd = np.ascontiguousarray(nodes, dtype=np.uint32)
        lp = None if logp is None else np.ascontiguousarray(logp, dtype=np.float64)
        h = C.c_void_p()
        _ffi.check(_ffi.lib().phmm_mappings_create(reads._h, _ptr(po), _ptr(nd), _ptr(lp), C.byref(h)))
        return Mappings(h, reads)

    def __del__(self):
        if getattr(self, "_h", None):
            _ffi.lib().phmm_mappings_destroy(self._h)
            self._h = None

    def arrays(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        if self._cache is None:
            L = _ffi.lib()
            tp, te = L.phmm_mappings_total_positions(self._h), L.phmm_mappings_total_entries(self._h)
            po = np.empty(tp + 1, dtype=np.uint64)
            nd = np.empty(max(te, 1), dtype=np.uint32)
            lp = np.empty(max(te, 1), dtype=np.float64)
            _ffi.check(L.phmm_mappings_export(self._h, _ptr(po), _ptr(nd), _ptr(lp)))
            self._cache = (po, nd[:te], lp[:te])
        return self._cache

    def nodes(self, read: int, pos: int) -> List[int]:
        po, nd, _ = self.arrays()
        g = int(self.reads.offsets[read]) + pos
        return nd[int(po[g]):int(po[g + 1])].tolist()

    def probs(self, read: int, pos: int) -> np.ndarray:
        po, _, lp = self.arrays()
        g = int(self.reads.offsets[read]) + pos
        return lp[int(po[g]):int(po[g + 1])]

    def read_logp(self, out_logp=None):
        """ln P(read) of the forward pass that produced these mappings -> (total, per read)."""
        lp = np.empty(len(self.reads)) if out_logp is None else out_logp
        tot = np.empty(1)
        _ffi.check(_ffi.lib().phmm_mappings_read_logp(self._h, _ptr(lp), _ptr(tot)))
        return float(tot[0]), lp

    def read_logp_backward(self, out_logp=None):
        """ln P(read) of the backward pass that produced these mappings (B.tables[0].mb,
        PHMMOutput::to_full_prob_backward) -> (total, per read)."""
        lp = np.empty(len(self.reads)) if out_logp is None else out_logp
        tot = np.empty(1)
        _ffi.check(_ffi.lib().phmm_mappings_read_logp_backward(self._h, _ptr(lp), _ptr(tot)))
        return float(tot[0]), lp

    def map_nodes(self, model_after: "PHMMModel", map_off: np.ndarray, map_nodes: np.ndarray) -> "Mappings":
        """Mapping::map_nodes (hint.rs:60-88) for every read: carry the lists over to another graph through a
        node map given as CSR over this mapping's graph (MultiDbg::hint_kp1_from_hint_k,
        PurgeEdgeMap::update_mapping)."""
        mo = np.ascontiguousarray(map_off, dtype=np.uint32)
        mn = np.ascontiguousarray(map_nodes, dtype=np.uint32)
        h = C.c_void_p()
        _ffi.check(_ffi.lib().phmm_mappings_map_nodes(model_after._h, self.reads._h, self._h, _ptr(mo), _ptr(mn),
                                                      mo.shape[0] - 1, C.byref(h)))
        return Mappings(h, self.reads)

    def to_node_freqs(self, n_nodes: int) -> np.ndarray:
        """Mappings::to_node_freqs (hint.rs:161-171)"""
        out = np.empty(n_nodes)
        _ffi.check(_ffi.lib().phmm_mappings_node_freqs(self._h, n_nodes, _ptr(out)))
        return out


class DenseTables:
    """PHMMTables of one read (natural-log values), tables[i] <-> x[i] (src/hmmv2.rs:7-29)."""

    def __init__(self, m, i, d, scal):
        self.m, self.i, self.d, self.scal = m, i, d, scal

    def __len__(self):
        return self.m.shape[0]

    @property
    def mb(self):
        return self.scal[:, 0]

    @property
    def ib(self):
        return self.scal[:, 1]

    @property
    def e(self):
        return self.scal[:, 2]


class ListTables:
    """The tables of the list pass (PHMMModel.run_with_mapping_tables, include/phmm_amd_tables.h): forward_with_mapping
    and backward_with_mapping of every read on its lists as the PHMMTables they are, natural logs, -inf = probability 0.

    Read r of length L, position p in 0..L-1, g = read_off[r] + p; entry a in [pos_off[g], pos_off[g+1]), v = nodes[a]:
      fwd[a] = ln F.tables[p].{m, i, d}[v],  fwd_scal[g] = ln F.tables[p].(ib, e)     (F.tables[p].mb is 0)
      bwd[a] = ln B.tables[p].{m, i, d}[v],  bwd_scal[g] = ln B.tables[p].(mb, ib)    (B.tables[p].e is 0)
    bwd is the table on list p, B.tables[p] -- not B.table_merged(p + 1), the one a posterior multiplies F.tables[p]
    with; table_merged() applies the reference's index rule.  A half that was not asked for is None.  Scalars are
    handed out as [mb, ib, e], the order of DenseTables.scal."""

    def __init__(self):
        self.read_off = self.pos_off = self.nodes = None
        self.fwd = self.fwd_scal = self.bwd = self.bwd_scal = None
        self.logp_forward = self.logp_backward = None
        self.p_end, self.n_nodes = 0.0, 0

    @staticmethod
    def from_arrays(read_off, pos_off, nodes, p_end: float, n_nodes: int, forward=None, forward_scalars=None,
                    backward=None, backward_scalars=None, logp_forward=None, logp_backward=None) -> "ListTables":
        """From the arrays of the call (or of any other source of the same tables); needs no GPU.  p_end: ln of the
        model's end probability and n_nodes: its node count, for b_init.  Totals that are not given are read off the
        scalars: ln F.tables[L-1].e and ln B.tables[0].mb."""
        t = ListTables()
        t.read_off = np.ascontiguousarray(read_off, dtype=np.uint64)
        t.pos_off = np.ascontiguousarray(pos_off, dtype=np.uint64)
        t.nodes = np.ascontiguousarray(nodes, dtype=np.uint32)
        tb, te = int(t.read_off[-1]), int(t.pos_off[-1])
        if t.pos_off.shape[0] != tb + 1 or t.nodes.shape[0] < te:
            raise ValueError("pos_off / nodes do not fit read_off")

        def plane(a, rows, cols):
            if a is None:
                return None
            a = np.asarray(a, dtype=np.float64)
            if a.shape != (rows, cols):
                raise ValueError(f"expected shape {(rows, cols)}, got {a.shape}")
            return a

        t.fwd, t.bwd = plane(forward, te, 3), plane(backward, te, 3)
        t.fwd_scal, t.bwd_scal = plane(forward_scalars, tb, 2), plane(backward_scalars, tb, 2)
        t.p_end, t.n_nodes = float(p_end), int(n_nodes)
        R = t.read_off.shape[0] - 1
        lens = (t.read_off[1:] - t.read_off[:-1]).astype(np.int64)
        if logp_forward is None and t.fwd_scal is not None:
            logp_forward = np.full(R, -np.inf)
            nz = lens > 0
            logp_forward[nz] = t.fwd_scal[t.read_off[1:][nz].astype(np.int64) - 1, 1]
        if logp_backward is None and t.bwd_scal is not None:
            logp_backward = np.full(R, -np.inf)
            nz = lens > 0
            logp_backward[nz] = t.bwd_scal[t.read_off[:-1][nz].astype(np.int64), 0]
        t.logp_forward = None if logp_forward is None else np.asarray(logp_forward, dtype=np.float64)
        t.logp_backward = None if logp_backward is None else np.asarray(logp_backward, dtype=np.float64)
        return t

    def __len__(self) -> int:
        return self.read_off.shape[0] - 1

    def read_len(self, read: int) -> int:
        return int(self.read_off[read + 1]) - int(self.read_off[read])

    def _span(self, read: int, pos: int):
        if not 0 <= pos < self.read_len(read):
            raise IndexError(f"position {pos} outside read {read}")
        g = int(self.read_off[read]) + pos
        return g, int(self.pos_off[g]), int(self.pos_off[g + 1])

    def forward(self, read: int, pos: int):
        """F.tables[pos] of the read -> (nodes[n], values[n, 3] = ln m, i, d, scalars = ln [mb, ib, e])"""
        g, a0, a1 = self._span(read, pos)
        vals = None if self.fwd is None else self.fwd[a0:a1]
        scal = None if self.fwd_scal is None else np.array([-np.inf, self.fwd_scal[g, 0], self.fwd_scal[g, 1]])
        return self.nodes[a0:a1], vals, scal

    def backward(self, read: int, pos: int):
        """B.tables[pos] of the read, the table on list pos -> (nodes[n], values[n, 3], scalars = ln [mb, ib, e])"""
        g, a0, a1 = self._span(read, pos)
        vals = None if self.bwd is None else self.bwd[a0:a1]
        scal = None if self.bwd_scal is None else np.array([self.bwd_scal[g, 0], self.bwd_scal[g, 1], -np.inf])
        return self.nodes[a0:a1], vals, scal

    def table_merged(self, kind: str, read: int, i: int):
        """PHMMTables::table_merged (table.rs:414-434) -> (nodes, values, scalars) as forward() / backward().
        'forward': index 0 is f_init (mb = 1, nothing else), index i >= 1 is F.tables[i - 1].
        'backward': index i >= L is b_init (p_end in every state of every node, nothing else), index i < L is B.tables[i].
        The two init tables are built from the parameters."""
        if kind == "forward":
            if i == 0:
                return (np.zeros(0, dtype=np.uint32), np.zeros((0, 3)), np.array([0.0, -np.inf, -np.inf]))
            return self.forward(read, i - 1)
        if kind == "backward":
            if i >= self.read_len(read):
                return (np.arange(self.n_nodes, dtype=np.uint32), np.full((self.n_nodes, 3), self.p_end),
                        np.array([-np.inf, -np.inf, -np.inf]))
            return self.backward(read, i)
        raise ValueError("kind must be 'forward' or 'backward'")

    def prefix_logp(self, read: int) -> np.ndarray:
        """ln F.tables[p].e for every base p: the likelihood of the prefix ending at base p"""
        return self.fwd_scal[int(self.read_off[read]):int(self.read_off[read + 1]), 1]

    def suffix_logp(self, read: int) -> np.ndarray:
        """ln B.tables[p].mb for every base p: the likelihood of the suffix from base p"""
        return self.bwd_scal[int(self.read_off[read]):int(self.read_off[read + 1]), 0]

    def ins_begin_posterior(self, read: int) -> np.ndarray:
        """ln of the posterior that base p was emitted from InsBegin, for every base p of the read:
        ln F.tables[p].ib + ln B.table_merged(p + 1).ib - ln P -- the ib scalar of to_emit_probs(p + 1).  -inf at the
        last base (b_init.ib = 0) and everywhere for a read of probability 0."""
        g0, g1 = int(self.read_off[read]), int(self.read_off[read + 1])
        out = np.full(g1 - g0, -np.inf)
        lp = float(self.logp_forward[read]) if g1 > g0 else -np.inf
        if g1 - g0 > 1 and lp > -np.inf:
            f, b = self.fwd_scal[g0:g1 - 1, 0], self.bwd_scal[g0 + 1:g1, 1]
            ok = (f > -np.inf) & (b > -np.inf)
            out[:-1][ok] = f[ok] + b[ok] - lp
        return out

    def top_states(self, kind: str, read: int, pos: int, n: int):
        """The first n entries of PHMMTable::to_states() (table.rs:215-254) of F.tables[pos] / B.tables[pos]: every
        Match in slot order, then every Ins, then every Del, sorted ascending by value (stable) and reversed -- among
        equal values Del before Ins before Match and the later slot first -> [(node, 'M' | 'I' | 'D', ln value), ...].
        This is what to_summary_string_n formats."""
        if kind not in ("forward", "backward"):
            raise ValueError("kind must be 'forward' or 'backward'")
        nodes, vals, _ = self.forward(read, pos) if kind == "forward" else self.backward(read, pos)
        k = nodes.shape[0]
        flat = vals.T.reshape(-1)  # Match.., Ins.., Del..
        order = np.argsort(flat, kind="stable")[::-1][:max(int(n), 0)]
        return [(int(nodes[j % k]), "MID"[j // k], float(flat[j])) for j in order.tolist()]


PATH_NONE = 0xFFFFFFFF       # PHMM_PATH_NONE (include/phmm_amd_path.h)
PATH_INS_BEGIN = 0xFFFFFFFD  # PHMM_PATH_INS_BEGIN


def path_states(mappings: "Mappings", read: int, path: np.ndarray) -> List[Tuple[Optional[int], str]]:
    """The rows of read `read` in the path of PHMMModel.run_with_mapping_best_path as the states the path passes, in
    order: [(node, kind), ...] with kind 'M', 'I' or 'D' and node = nodes[pos_off[g] + slot] of the mappings' CSR, or
    (None, 'IB') for InsBegin.  Empty for a read without a path."""
    po, nd, _ = mappings.arrays()
    g0, g1 = int(mappings.reads.offsets[read]), int(mappings.reads.offsets[read + 1])
    out: List[Tuple[Optional[int], str]] = []
    for g in range(g0, g1):
        for code in path[g].tolist():
            if code == PATH_NONE:
                break
            if code == PATH_INS_BEGIN:
                out.append((None, "IB"))
            else:
                out.append((int(nd[int(po[g]) + (code >> 2)]), "MID"[code & 3]))
    return out


class Alignments:
    """The alignment records of PHMMModel.run_with_mapping_alignments (include/phmm_amd_align.h): per alignment
    a = read * max(n_samples, 1) + sample a CIGAR -- runs (len, op) over the path's events, op 7 '=', 8 'X', 1 'I',
    2 'D' -- and a node walk -- runs (first node, len) of consecutive node ids over its Match and Del states.  The
    records stay on the device until arrays() is first called."""

    def __init__(self, handle, n_reads: int, n_samples: int):
        self._h = handle
        self.n_reads, self.n_samples = int(n_reads), int(n_samples)
        self._cache = None

    @staticmethod
    def from_arrays(n_reads: int, n_samples: int, op_off, ops, run_off, run_node, run_len) -> "Alignments":
        """records that are on the host already (a file read back, a test)"""
        a = Alignments(None, n_reads, n_samples)
        a._cache = (np.asarray(op_off, dtype=np.uint64), np.asarray(ops, dtype=np.uint32),
                    np.asarray(run_off, dtype=np.uint64), np.asarray(run_node, dtype=np.uint32),
                    np.asarray(run_len, dtype=np.uint32))
        assert a._cache[0].shape[0] == len(a) + 1 == a._cache[2].shape[0]
        return a

    def __del__(self):
        if getattr(self, "_h", None):
            from . import _ffi_align
            _ffi_align.lib().phmm_alignments_destroy(self._h)
            self._h = None

    def __len__(self) -> int:
        return self.n_reads * max(self.n_samples, 1)

    def index(self, read: int, sample: int = 0) -> int:
        return read * max(self.n_samples, 1) + sample

    def arrays(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """(op_off[A + 1], ops, run_off[A + 1], run_node, run_len), copied from the device on the first call"""
        if self._cache is None:
            from . import _ffi_align
            L = _ffi_align.lib()
            A, n_ops, n_runs = (int(L.phmm_alignments_count(self._h)), int(L.phmm_alignments_total_ops(self._h)),
                                int(L.phmm_alignments_total_runs(self._h)))
            op_off, run_off = np.empty(A + 1, dtype=np.uint64), np.empty(A + 1, dtype=np.uint64)
            ops, rn, rl = (np.empty(max(n_ops, 1), dtype=np.uint32), np.empty(max(n_runs, 1), dtype=np.uint32),
                           np.empty(max(n_runs, 1), dtype=np.uint32))
            _ffi.check(L.phmm_alignments_export(self._h, _ptr(op_off), _ptr(ops), _ptr(run_off), _ptr(rn), _ptr(rl)))
            self._cache = (op_off, ops[:n_ops], run_off, rn[:n_runs], rl[:n_runs])
        return self._cache

    def cigar(self, a: int) -> List[Tuple[int, int]]:
        op_off, ops = self.arrays()[:2]
        return [(w >> 4, w & 15) for w in ops[int(op_off[a]):int(op_off[a + 1])].tolist()]

    def cigar_string(self, a: int) -> str:
        from ._ffi_align import OP_CHARS
        return "".join(f"{n}{OP_CHARS[op]}" for n, op in self.cigar(a))

    def walk(self, a: int) -> List[Tuple[int, int]]:
        _, _, run_off, rn, rl = self.arrays()
        e0, e1 = int(run_off[a]), int(run_off[a + 1])
        return list(zip(rn[e0:e1].tolist(), rl[e0:e1].tolist()))

    def nodes(self, a: int) -> List[int]:
        return [v for first, n in self.walk(a) for v in range(first, first + n)]

    def states(self, a: int) -> List[Tuple[Optional[int], str]]:
        """the (node, kind) sequence path_states gives for the alignment's read and plane: =, X and D take one step of
        the walk each; an I sits on the last step's node, or is InsBegin before the first step"""
        steps = iter(self.nodes(a))
        out: List[Tuple[Optional[int], str]] = []
        last = None
        for n, op in self.cigar(a):
            for _ in range(n):
                if op == 1:
                    out.append((None, "IB") if last is None else (last, "I"))
                else:
                    last = next(steps)
                    out.append((last, "D" if op == 2 else "M"))
        return out


class ReadUsage:
    """The rows of PHMMModel.run_with_mapping_read_usage (include/phmm_amd_usage.h): per read the distinct keys (nodes,
    or node groups) among its list entries in ascending order and, per key, the summed posterior of the read's Match,
    Ins and Del states there -- PHMMOutput::to_state_probs() of the read, kept sparse.  CSR over the reads; the rows
    stay on the device until arrays() is first called.  totals[K, 3]: the column sums over all reads (None if the call
    did not ask for them)."""

    def __init__(self, handle, n_reads: int, n_keys: int, totals=None):
        self._h = handle
        self.n_reads, self.n_keys = int(n_reads), int(n_keys)
        self.totals = totals
        self._cache = None
        self._by_key = None

    @staticmethod
    def from_arrays(n_keys: int, row_off, keys, usage, totals=None) -> "ReadUsage":
        """rows that are on the host already (a file read back, a test)"""
        row_off = np.asarray(row_off, dtype=np.uint64)
        u = ReadUsage(None, row_off.shape[0] - 1, n_keys, totals)
        u._cache = (row_off, np.asarray(keys, dtype=np.uint32), np.asarray(usage, dtype=np.float64).reshape(-1, 3))
        assert int(row_off[-1]) == u._cache[1].shape[0] == u._cache[2].shape[0]
        return u

    def __del__(self):
        if getattr(self, "_h", None):
            from . import _ffi_usage
            _ffi_usage.lib().phmm_read_usage_destroy(self._h)
            self._h = None

    def __len__(self) -> int:
        return self.n_reads

    def arrays(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(row_off[R + 1], keys[total], usage[total, 3]), copied from the device on the first call"""
        if self._cache is None:
            from . import _ffi_usage
            L = _ffi_usage.lib()
            R, total = int(L.phmm_read_usage_reads(self._h)), int(L.phmm_read_usage_total(self._h))
            row_off = np.empty(R + 1, dtype=np.uint64)
            keys, usage = np.empty(max(total, 1), dtype=np.uint32), np.empty((max(total, 1), 3))
            _ffi.check(L.phmm_read_usage_export(self._h, _ptr(row_off), _ptr(keys), _ptr(usage)))
            self._cache = (row_off, keys[:total], usage[:total])
        return self._cache

    def row(self, r: int) -> Tuple[np.ndarray, np.ndarray]:
        """(keys[n], usage[n, 3]) of read r"""
        row_off, keys, usage = self.arrays()
        e0, e1 = int(row_off[r]), int(row_off[r + 1])
        return keys[e0:e1], usage[e0:e1]

    def state_probs(self, r: int) -> np.ndarray:
        """dense [K, 3]: to_state_probs() of read r (Match, Ins, Del per key)"""
        keys, usage = self.row(r)
        out = np.zeros((self.n_keys, 3))
        out[keys] = usage
        return out

    def node_freqs(self, r: int) -> np.ndarray:
        """dense [K]: the reference's to_node_freqs() of read r, (Match + Ins) + Del per key"""
        keys, usage = self.row(r)
        out = np.zeros(self.n_keys)
        out[keys] = usage[:, 0] + usage[:, 1] + usage[:, 2]
        return out

    def reads_of(self, key: int) -> Tuple[np.ndarray, np.ndarray]:
        """(reads[n], usage[n, 3]): the reads whose row holds the key, in ascending order, and their entries -- the
        transpose of row()"""
        row_off, keys, usage = self.arrays()
        if self._by_key is None:
            read_of = np.repeat(np.arange(self.n_reads, dtype=np.int64), np.diff(row_off.astype(np.int64)))
            order = np.argsort(keys, kind="stable")
            self._by_key = (order, keys[order], read_of)
        order, sorted_keys, read_of = self._by_key
        e0, e1 = np.searchsorted(sorted_keys, key, side="left"), np.searchsorted(sorted_keys, key, side="right")
        sel = order[e0:e1]
        return read_of[sel], usage[sel]


class ReadEdges:
    """The rows of PHMMModel.run_with_mapping_read_edges (include/phmm_amd_edges.h): per read the distinct keys (edges and
    Begin transitions, or the keys of the caller's map) among the nonzero transition terms of the read in ascending
    order and, per key, their sum -- PHMMOutput::to_edge_and_init_freqs() of the read, kept sparse.  A key absent from a
    row counts as 0.  CSR over the reads; the rows stay on the device until arrays() is first called.  totals[K]: the
    column sums over all reads (None if the call did not ask for them); end_terms[R, 2]: (A_r, T_r), the two scalars
    behind the Begin terms every read has on all nodes at its last base, which are not row entries.  n_edges: E of the
    model under the default keys (key e = edge e, key E + v = Begin -> v), None under a caller's map."""

    def __init__(self, handle, n_reads: int, n_keys: int, totals=None, end_terms=None, n_edges: Optional[int] = None):
        self._h = handle
        self.n_reads, self.n_keys = int(n_reads), int(n_keys)
        self.totals, self.end_terms = totals, end_terms
        self.n_edges = None if n_edges is None else int(n_edges)
        self._cache = None
        self._by_key = None

    @staticmethod
    def from_arrays(n_keys: int, row_off, keys, usage, totals=None, end_terms=None, n_edges: Optional[int] = None) -> "ReadEdges":
        """rows that are on the host already (a file read back, a test)"""
        row_off = np.asarray(row_off, dtype=np.uint64)
        u = ReadEdges(None, row_off.shape[0] - 1, n_keys, totals, end_terms, n_edges)
        u._cache = (row_off, np.asarray(keys, dtype=np.uint32), np.asarray(usage, dtype=np.float64).reshape(-1))
        assert int(row_off[-1]) == u._cache[1].shape[0] == u._cache[2].shape[0]
        return u

    def __del__(self):
        if getattr(self, "_h", None):
            from . import _ffi_edges
            _ffi_edges.lib().phmm_read_edges_destroy(self._h)
            self._h = None

    def __len__(self) -> int:
        return self.n_reads

    def arrays(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(row_off[R + 1], keys[total], usage[total]), copied from the device on the first call"""
        if self._cache is None:
            from . import _ffi_edges
            L = _ffi_edges.lib()
            R, total = int(L.phmm_read_edges_reads(self._h)), int(L.phmm_read_edges_total(self._h))
            row_off = np.empty(R + 1, dtype=np.uint64)
            keys, usage = np.empty(max(total, 1), dtype=np.uint32), np.empty(max(total, 1))
            _ffi.check(L.phmm_read_edges_export(self._h, _ptr(row_off), _ptr(keys), _ptr(usage)))
            self._cache = (row_off, keys[:total], usage[:total])
        return self._cache

    export = arrays

    def row(self, r: int) -> Tuple[np.ndarray, np.ndarray]:
        """(keys[n], usage[n]) of read r"""
        row_off, keys, usage = self.arrays()
        e0, e1 = int(row_off[r]), int(row_off[r + 1])
        return keys[e0:e1], usage[e0:e1]

    def key_freqs(self, r: int) -> np.ndarray:
        """dense [K]: the row of read r, 0 where a key is absent"""
        keys, usage = self.row(r)
        out = np.zeros(self.n_keys)
        out[keys] = usage
        return out

    def _default_keys(self) -> int:
        if self.n_edges is None:
            raise ValueError("the rows are keyed by a caller's map: edge_freqs / init_freqs need the default keys")
        return self.n_edges

    def edge_freqs(self, r: int) -> np.ndarray:
        """dense [E]: the edge half of to_edge_and_init_freqs() of read r (default keys only)"""
        return self.key_freqs(r)[:self._default_keys()]

    def init_freqs(self, r: int, arrays, last_base: int) -> np.ndarray:
        """dense [N]: the Begin half of to_edge_and_init_freqs() of read r with the end terms added (default keys only):
        row value at key E + v + init_v (A_r + T_r e_v(last_base)); arrays: the model's PHMMArrays, last_base: the
        read's last base as a byte value"""
        E = self._default_keys()
        if self.end_terms is None:
            raise ValueError("the call did not return end terms")
        par = arrays.param
        init = np.exp(np.asarray(arrays.init_logp, dtype=np.float64))
        e = np.where(np.asarray(arrays.emission) == int(last_base), math.exp(par.p_match), math.exp(par.p_mismatch))
        a_r, t_r = float(self.end_terms[r, 0]), float(self.end_terms[r, 1])
        return self.key_freqs(r)[E:] + init * (a_r + t_r * e)

    def reads_of(self, key: int) -> Tuple[np.ndarray, np.ndarray]:
        """(reads[n], usage[n]): the reads whose row holds the key, in ascending order, and their entries -- the
        transpose of row()"""
        row_off, keys, usage = self.arrays()
        if self._by_key is None:
            read_of = np.repeat(np.arange(self.n_reads, dtype=np.int64), np.diff(row_off.astype(np.int64)))
            order = np.argsort(keys, kind="stable")
            self._by_key = (order, keys[order], read_of)
        order, sorted_keys, read_of = self._by_key
        e0, e1 = np.searchsorted(sorted_keys, key, side="left"), np.searchsorted(sorted_keys, key, side="right")
        sel = order[e0:e1]
        return read_of[sel], usage[sel]


def base_codes(bases) -> np.ndarray:
    """bytes or u8[.] of ASCII bases -> int64 codes A 0, C 1, G 2, T 3, anything else -1"""
    b = np.frombuffer(bases, dtype=np.uint8) if isinstance(bases, (bytes, bytearray)) else np.asarray(bases, dtype=np.uint8)
    code = np.full(256, -1, dtype=np.int64)
    code[np.frombuffer(b"ACGT", dtype=np.uint8)] = np.arange(4)
    return code[b]


class Pileup:
    """The result of PHMMModel.run_with_mapping_pileup (include/phmm_amd_pileup.h): a pileup on the graph.  The rows
    are those of a ReadUsage under the key 4 * node + base code (A 0, C 1, G 2, T 3): per read the distinct (node, read
    base) pairs among its list entries in ascending order and, per pair, the summed posterior of the read's Match, Ins
    and Del states at that node at the positions showing that base.  CSR over the reads; the rows stay on the device
    until arrays() is first called.  totals[N, 9]: per node the Match mass by read base (columns 0-3), the Ins mass by
    read base (4-7) and the Del mass (8) over all reads; summed from the rows on the host when the call did not ask
    for them.  The Del value of a row entry is the Del mass at the positions of that base: only its sum over the four
    bases has a meaning of its own."""

    def __init__(self, handle, n_reads: int, n_nodes: int, totals=None):
        self._h = handle
        self.n_reads, self.n_nodes = int(n_reads), int(n_nodes)
        self._totals = totals
        self._cache = None
        self._by_key = None

    @staticmethod
    def from_arrays(n_nodes: int, row_off, keys, usage, totals=None) -> "Pileup":
        """rows that are on the host already (a file read back, a test)"""
        row_off = np.asarray(row_off, dtype=np.uint64)
        u = Pileup(None, row_off.shape[0] - 1, n_nodes, None if totals is None else np.asarray(totals, dtype=np.float64))
        u._cache = (row_off, np.asarray(keys, dtype=np.uint32), np.asarray(usage, dtype=np.float64).reshape(-1, 3))
        assert int(row_off[-1]) == u._cache[1].shape[0] == u._cache[2].shape[0]
        assert u._cache[1].size == 0 or int(u._cache[1].max()) < 4 * u.n_nodes
        assert u._totals is None or u._totals.shape == (u.n_nodes, 9)
        return u

    def __del__(self):
        if getattr(self, "_h", None):
            from . import _ffi_usage
            _ffi_usage.lib().phmm_read_usage_destroy(self._h)
            self._h = None

    def __len__(self) -> int:
        return self.n_reads

    def arrays(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(row_off[R + 1], keys[total], usage[total, 3]), copied from the device on the first call"""
        if self._cache is None:
            if not self._h:
                raise ValueError("the call kept no rows (want_rows=False)")
            from . import _ffi_usage
            L = _ffi_usage.lib()
            R, total = int(L.phmm_read_usage_reads(self._h)), int(L.phmm_read_usage_total(self._h))
            row_off = np.empty(R + 1, dtype=np.uint64)
            keys, usage = np.empty(max(total, 1), dtype=np.uint32), np.empty((max(total, 1), 3))
            _ffi.check(L.phmm_read_usage_export(self._h, _ptr(row_off), _ptr(keys), _ptr(usage)))
            self._cache = (row_off, keys[:total], usage[:total])
        return self._cache

    @property
    def totals(self) -> np.ndarray:
        """[N, 9]: Match by read base, Ins by read base, Del"""
        if self._totals is None:
            _, keys, usage = self.arrays()
            k = keys.astype(np.int64)
            t = np.zeros((self.n_nodes, 9))
            np.add.at(t, (k >> 2, k & 3), usage[:, 0])
            np.add.at(t, (k >> 2, 4 + (k & 3)), usage[:, 1])
            np.add.at(t[:, 8], k >> 2, usage[:, 2])
            self._totals = t
        return self._totals

    def row(self, r: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(nodes[n], base_codes[n], usage[n, 3]) of read r, ascending by (node, base code)"""
        row_off, keys, usage = self.arrays()
        e0, e1 = int(row_off[r]), int(row_off[r + 1])
        return keys[e0:e1] >> 2, keys[e0:e1] & 3, usage[e0:e1]

    def reads_of(self, node: int, base: int) -> Tuple[np.ndarray, np.ndarray]:
        """(reads[n], usage[n, 3]): the reads that list the node at a position showing the base (code 0..3), in
        ascending order, and their entries: which reads carry which allele at the node"""
        row_off, keys, usage = self.arrays()
        if self._by_key is None:
            read_of = np.repeat(np.arange(self.n_reads, dtype=np.int64), np.diff(row_off.astype(np.int64)))
            order = np.argsort(keys, kind="stable")
            self._by_key = (order, keys[order], read_of)
        order, sorted_keys, read_of = self._by_key
        key = 4 * int(node) + int(base)
        e0, e1 = np.searchsorted(sorted_keys, key, side="left"), np.searchsorted(sorted_keys, key, side="right")
        sel = order[e0:e1]
        return read_of[sel], usage[sel]

    @property
    def match_counts(self) -> np.ndarray:
        """[N, 4]: the Match mass per node and read base"""
        return self.totals[:, 0:4]

    @property
    def ins_counts(self) -> np.ndarray:
        """[N, 4]: the Ins mass per node and inserted base"""
        return self.totals[:, 4:8]

    @property
    def del_counts(self) -> np.ndarray:
        """[N]: the Del mass per node"""
        return self.totals[:, 8]

    def depth(self) -> np.ndarray:
        """[N]: the Match mass per node, summed over the read bases"""
        return self.match_counts.sum(axis=1)

    def consensus(self) -> np.ndarray:
        """[N] int64: the code of the heaviest Match base per node (the first of equals), -1 where the depth is 0"""
        m = self.match_counts
        return np.where(self.depth() > 0, np.argmax(m, axis=1), -1).astype(np.int64)

    def disagreements(self, emission, min_mass: float, min_share: float = 0.5) -> np.ndarray:
        """the nodes whose heaviest Match base is not their emission (ASCII, u8[N] or bytes), carries at least min_mass
        and makes up at least min_share of the node's depth: where the reads agree with each other against the graph"""
        e = base_codes(emission)
        assert e.shape[0] == self.n_nodes
        m, top, depth = self.match_counts, self.consensus(), self.depth()
        mass = m[np.arange(self.n_nodes), np.maximum(top, 0)]
        return np.nonzero((top >= 0) & (top != e) & (mass >= min_mass) & (mass >= min_share * depth))[0]

    def error_profile(self, emission) -> dict:
        """{"mismatch", "ins", "del"}: the shares of the summed Match + Ins + Del mass that are Match mass under a read
        base other than the node's emission, Ins mass and Del mass (a node whose emission is none of A C G T adds no
        mismatch); zeros for an empty pileup"""
        e = base_codes(emission)
        assert e.shape[0] == self.n_nodes
        m = self.match_counts
        ok = e >= 0
        agree = float(m[ok, e[ok]].sum())
        mismatch = float(m[ok].sum()) - agree
        ins, dele = float(self.ins_counts.sum()), float(self.del_counts.sum())
        total = float(m.sum()) + ins + dele
        if total <= 0.0:
            return {"mismatch": 0.0, "ins": 0.0, "del": 0.0}
        return {"mismatch": mismatch / total, "ins": ins / total, "del": dele / total}


class PHMMModel:
    """PHMMModel<N, E> (src/hmmv2/common.rs:61-64) resident on one MI355X."""

    def __init__(self, arrays: PHMMArrays):
        self.arrays = arrays
        self.param = arrays.param
        self._cp = arrays.param.to_c()
        em = np.ascontiguousarray(arrays.emission, dtype=np.uint8)
        init = np.ascontiguousarray(arrays.init_logp, dtype=np.float64)
        src = np.ascontiguousarray(arrays.edge_src, dtype=np.uint32)
        dst = np.ascontiguousarray(arrays.edge_dst, dtype=np.uint32)
        tr = np.ascontiguousarray(arrays.trans_logp, dtype=np.float64)
        self.n_nodes, self.n_edges = em.shape[0], src.shape[0]
        h = C.c_void_p()
        _ffi.check(_ffi.lib().phmm_model_create(self.n_nodes, self.n_edges, _ptr(em), _ptr(init), _ptr(src),
                                                _ptr(dst), _ptr(tr), C.byref(self._cp), C.byref(h)))
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            _ffi.lib().phmm_model_destroy(self._h)
            self._h = None

    def set_probs(self, init_logp: np.ndarray, trans_logp: np.ndarray) -> None:
        """next candidate copy-number vector on the same topology (posterior.rs:483-501)"""
        a = np.ascontiguousarray(init_logp, dtype=np.float64)
        b = np.ascontiguousarray(trans_logp, dtype=np.float64)
        assert a.shape[0] == self.n_nodes and b.shape[0] == self.n_edges
        _ffi.check(_ffi.lib().phmm_model_set_probs(self._h, _ptr(a), _ptr(b)))

    # ---- dense: forward / backward / run (forward.rs:24-45, backward.rs:24-53, freq.rs:42-46)
    def _tables(self, read: bytes, want_f: bool, want_b: bool):
        r = np.frombuffer(bytes(read), dtype=np.uint8)
        L, N = r.shape[0], self.n_nodes
        if L == 0:
            raise _ffi.PhmmError(_ffi.PHMM_EINVAL, "empty read")
        f = [np.empty((L, N)) for _ in range(3)] + [np.empty((L, 3))] if want_f else [None] * 4
        b = [np.empty((L, N)) for _ in range(3)] + [np.empty((L, 3))] if want_b else [None] * 4
        _ffi.check(_ffi.lib().phmm_dense_tables(self._h, _ptr(r), L, *[_ptr(x) for x in f], *[_ptr(x) for x in b]))
        return (DenseTables(*f) if want_f else None, DenseTables(*b) if want_b else None)

    def forward(self, read: bytes) -> DenseTables:
        return self._tables(read, True, False)[0]

    def backward(self, read: bytes) -> DenseTables:
        return self._tables(read, False, True)[1]

    def run(self, read: bytes) -> "PHMMOutput":
        f, b = self._tables(read, True, True)
        return PHMMOutput(self, bytes(read), f, b)

    def backward_sparse(self, read: bytes):
        """PHMMModel::backward_sparse (backward.rs:146-185) of one read -> (DenseTables with -inf where the
        reference's sparse table holds no element, is_dense[L])."""
        r = np.frombuffer(bytes(read), dtype=np.uint8)
        L, N = r.shape[0], self.n_nodes
        if L == 0:
            raise _ffi.PhmmError(_ffi.PHMM_EINVAL, "empty read")
        b = [np.empty((L, N)) for _ in range(3)] + [np.empty((L, 3))]
        dense = np.zeros(L, dtype=np.uint8)
        _ffi.check(_ffi.lib().phmm_backward_sparse_tables(self._h, _ptr(r), L, *[_ptr(x) for x in b], _ptr(dense)))
        return DenseTables(*b), dense.astype(bool)

    def run_sparse(self, reads: ReadCollection):
        """PHMMModel::run_sparse (freq.rs:51-55) over a read set -> (ln P forward[R], ln P backward[R],
        node_freq[N] summed over the reads)."""
        lf, lb, nf = np.empty(len(reads)), np.empty(len(reads)), np.empty(self.n_nodes)
        _ffi.check(_ffi.lib().phmm_run_sparse(self._h, reads._h, _ptr(lf), _ptr(lb), _ptr(nf)))
        return lf, lb, nf

    def to_full_prob_sparse_backward(self, reads: ReadCollection):
        """PHMMModel::to_full_prob_sparse_backward (freq.rs:153-163) -> (total ln P, per-read ln P)."""
        lp = np.empty(len(reads))
        tot = np.empty(1)
        _ffi.check(_ffi.lib().phmm_full_prob_sparse_backward(self._h, reads._h, _ptr(lp), _ptr(tot)))
        return float(tot[0]), lp

    # ---- read-set drivers
    def run_dense(self, reads: ReadCollection, want_backward: bool = True, want_freq: bool = True,
                  out_logp=None, out_logp_backward=None, out_node_freq=None):
        """`run` over a read set + to_full_prob_forward/backward + summed to_node_freqs
        (freq.rs:89-119, 245-255).  Output buffers may be numpy arrays or torch tensors
        (host or device); they are allocated as numpy when omitted."""
        R, N = len(reads), self.n_nodes
        lf = np.empty(R) if out_logp is None else out_logp
        lb = (np.empty(R) if out_logp_backward is None else out_logp_backward) if want_backward else None
        nf = (np.empty(N) if out_node_freq is None else out_node_freq) if want_freq else None
        _ffi.check(_ffi.lib().phmm_run_dense(self._h, reads._h, _ptr(lf), _ptr(lb), _ptr(nf)))
        return lf, lb, nf

    def to_full_prob_reads(self, reads: ReadCollection, mappings: Optional[Mappings] = None,
                           use_max_ratio: bool = True, out_logp=None):
        """PHMMModel::to_full_prob_reads (freq.rs:175-192) -> (total ln P(R|G), per-read ln P)."""
        lp = np.empty(len(reads)) if out_logp is None else out_logp
        tot = np.empty(1)
        _ffi.check(_ffi.lib().phmm_full_prob_reads(self._h, reads._h, mappings._h if mappings else None,
                                                   int(use_max_ratio), _ptr(lp), _ptr(tot)))
        return float(tot[0]), lp

    def to_full_prob_reads_candidates(self, reads: ReadCollection, mappings: Mappings, init_logp: np.ndarray,
                                      trans_logp: np.ndarray):
        """candidate-batched likelihood (posterior.rs:483-515): init [C,N], trans [C,E]."""
        a = np.ascontiguousarray(init_logp, dtype=np.float64)
        b = np.ascontiguousarray(trans_logp, dtype=np.float64)
        Cn = a.shape[0]
        lp = np.empty((Cn, len(reads)))
        tot = np.empty(Cn)
        _ffi.check(_ffi.lib().phmm_full_prob_reads_candidates(self._h, reads._h, mappings._h, Cn, _ptr(a), _ptr(b),
                                                              _ptr(lp), _ptr(tot)))
        return tot, lp

    def run_dense_edge_freqs(self, reads: ReadCollection):
        """PHMMOutput::to_edge_and_init_freqs (freq.rs:276-298) summed over the reads
        -> (per-read ln P, edge_freq[E], init_freq[N])."""
        lf, ef, nf = np.empty(len(reads)), np.empty(max(self.n_edges, 1)), np.empty(self.n_nodes)
        _ffi.check(_ffi.lib().phmm_run_dense_edges(self._h, reads._h, _ptr(lf), _ptr(ef), _ptr(nf)))
        return lf, ef[:self.n_edges], nf

    def run_with_mapping_edge_freqs(self, reads: ReadCollection, mappings: Mappings):
        """PHMMModel::run_with_mapping (freq.rs:72-76) of every read on its lists, then
        PHMMOutput::to_edge_and_init_freqs (freq.rs:276-298) summed over the reads
        -> (per-read ln P, edge_freq[E], init_freq[N])."""
        lf, ef, nf = np.empty(len(reads)), np.empty(max(self.n_edges, 1)), np.empty(self.n_nodes)
        _ffi.check(_ffi.lib().phmm_run_with_mapping_edges(self._h, reads._h, mappings._h, _ptr(lf), _ptr(ef), _ptr(nf)))
        return lf, ef[:self.n_edges], nf

    def run_with_mapping_states(self, reads: ReadCollection, mappings: Mappings, want_states: bool = True,
                                want_best: bool = True):
        """PHMMModel::run_with_mapping (freq.rs:72-76) of every read on its lists, then per read position p
        PHMMOutput::to_emit_probs(p + 1) by state (table.rs:500-505) over the entries of the input lists and the head
        of its to_states() (table.rs:215-254)
        -> (per-read ln P, state_logp[total_entries, 3] | None, best[total_bases] | None).
        state_logp[a] = ln of Match, Ins, Del of entry a of the mappings' CSR (-inf: probability 0);
        best[g] = (slot << 2) | kind (0 Match, 1 Ins, 2 Del) of the position's largest value -- among equal values Del
        before Ins before Match, then the later slot --, 0xffffffff where no value is finite."""
        L = _ffi.lib()
        te = int(L.phmm_mappings_total_entries(mappings._h))
        lf = np.empty(len(reads))
        sl = np.empty((te, 3)) if want_states else None
        best = np.empty(reads.total_bases(), dtype=np.uint32) if want_best else None
        _ffi.check(L.phmm_run_with_mapping_states(self._h, reads._h, mappings._h, _ptr(lf),
                                                  _ptr(sl) if want_states and te else None,
                                                  _ptr(best) if want_best and best.size else None))
        return lf, sl, best

    def run_with_mapping_best_path(self, reads: ReadCollection, mappings: Mappings, want_path: bool = True):
        """The best path (Viterbi) of every read over its lists: forward_with_mapping (forward.rs:51-75) with every sum
        replaced by a maximum, and the walk back (include/phmm_amd_path.h)
        -> (logp[R], path[total_bases, stride] | None, counts[R, 4]).
        logp[r] = ln P of the best path (-inf: none); stride = n_max_gaps + 2; row g of path: entry 0 the emitting state
        of the base, (slot << 2) | 0 Match / 1 Ins or PATH_INS_BEGIN, then the Del states behind it as (slot << 2) | 2,
        then PATH_NONE; counts = matches, mismatches, insertions, deletions of the path.  path_states() turns the rows
        of one read into (node, kind) pairs."""
        R = len(reads)
        stride = int(self.param.n_max_gaps) + 2
        lp = np.empty(R)
        counts = np.empty((R, 4), dtype=np.uint32)
        path = np.empty((reads.total_bases(), stride), dtype=np.uint32) if want_path else None
        _ffi.check(_ffi.lib().phmm_run_with_mapping_best_path(self._h, reads._h, mappings._h, _ptr(lp),
                                                               _ptr(path) if want_path and path.size else None,
                                                               _ptr(counts)))
        return lp, path, counts

    def run_with_mapping_weighted_path(self, reads: ReadCollection, mappings: Mappings, weights, ib_weight=None,
                                       want_path: bool = True):
        """The legal walk of the largest summed weight of every read over its lists (include/phmm_amd_mea.h): the path
        family, the tie rule and the rows of run_with_mapping_best_path, with the model's logs deciding only which
        transitions exist and the value of a path being the sum, left to right, of the caller's weights
        -> (score[R], path[total_bases, stride] | None, counts[R, 4]).
        weights[total_entries, 3]: one finite double per entry of the mappings' CSR and kind (Match, Ins, Del), the
        layout of run_with_mapping_states' state_logp; ib_weight[total_bases]: the weight of InsBegin emitting each
        base (None: 0).  Both may be numpy arrays or torch tensors, host or device.  score[r] = -inf: no legal path."""
        from . import _ffi_mea
        R = len(reads)
        stride = int(self.param.n_max_gaps) + 2
        if isinstance(weights, np.ndarray):
            weights = np.ascontiguousarray(weights, dtype=np.float64)
        if isinstance(ib_weight, np.ndarray):
            ib_weight = np.ascontiguousarray(ib_weight, dtype=np.float64)
        score = np.empty(R)
        counts = np.empty((R, 4), dtype=np.uint32)
        path = np.empty((reads.total_bases(), stride), dtype=np.uint32) if want_path else None
        _ffi.check(_ffi_mea.lib().phmm_run_with_mapping_weighted_path(
            self._h, reads._h, mappings._h, _ptr(weights), _ptr(ib_weight), _ptr(score),
            _ptr(path) if want_path and path.size else None, _ptr(counts)))
        return score, path, counts

    def run_with_mapping_mea_path(self, reads: ReadCollection, mappings: Mappings, del_weight: float = 1.0,
                                  want_path: bool = True, want_weights: bool = False):
        """The maximum-expected-accuracy path of every read over its lists (include/phmm_amd_mea.h): the legal walk
        whose states have the largest summed posterior -- run_with_mapping_states with its values kept on the device,
        exp of them as weights (the Del column times del_weight, InsBegin 0), then run_with_mapping_weighted_path
        -> (logp_forward[R], score[R], path[total_bases, stride] | None, counts[R, 4], weights[total_entries, 3] | None).
        At del_weight = 1 the score is the expected number of the path's states, emitting and Del, that the true path
        shares at the same base; at 0 it counts emitting states only.  The rows are those of run_with_mapping_best_path,
        so path_states() works on them; weights are the ones used (feeding them to run_with_mapping_weighted_path gives
        the same bits)."""
        from . import _ffi_mea
        L = _ffi.lib()
        R, te = len(reads), int(L.phmm_mappings_total_entries(mappings._h))
        stride = int(self.param.n_max_gaps) + 2
        lf, score = np.empty(R), np.empty(R)
        counts = np.empty((R, 4), dtype=np.uint32)
        path = np.empty((reads.total_bases(), stride), dtype=np.uint32) if want_path else None
        w = np.empty((te, 3)) if want_weights else None
        _ffi.check(_ffi_mea.lib().phmm_run_with_mapping_mea_path(
            self._h, reads._h, mappings._h, float(del_weight), _ptr(lf), _ptr(score),
            _ptr(path) if want_path and path.size else None, _ptr(counts), _ptr(w) if want_weights and te else None))
        return lf, score, path, counts, w

    def run_with_mapping_tables(self, reads: ReadCollection, mappings: Mappings, want_forward: bool = True,
                                want_backward: bool = True) -> "ListTables":
        """PHMMModel::forward_with_mapping (forward.rs:51-75) and backward_with_mapping (backward.rs:59-93) of every
        read on its lists, with the tables themselves returned (include/phmm_amd_tables.h) -> ListTables: per list entry
        ln m, i, d of F.tables[p] and of B.tables[p], per base ln (ib, e) of F and ln (mb, ib) of B, per read
        ln F.tables[L-1].e and ln B.tables[0].mb.  A half that is not wanted is not run and its arrays are None.
        A read of probability 0 on its lists is a result: its values are -inf from where the mass ends."""
        from . import _ffi_tables
        L = _ffi.lib()
        R, tb = len(reads), reads.total_bases()
        te = int(L.phmm_mappings_total_entries(mappings._h))
        po, nd, _ = mappings.arrays()

        def half(want):
            if not want:
                return None, None, None
            return np.empty(R), np.empty((te, 3)), np.empty((tb, 2))

        lf, f, fs = half(want_forward)
        lb, b, bs = half(want_backward)
        _ffi.check(_ffi_tables.lib().phmm_run_with_mapping_tables(
            self._h, reads._h, mappings._h, _ptr(lf), _ptr(lb), _ptr(f) if f is not None and te else None,
            _ptr(fs) if fs is not None and tb else None, _ptr(b) if b is not None and te else None,
            _ptr(bs) if bs is not None and tb else None))
        return ListTables.from_arrays(reads.offsets, po, nd, self.param.p_end, self.n_nodes, f, fs, b, bs, lf, lb)

    def run_with_mapping_sample_paths(self, reads: ReadCollection, mappings: Mappings, n_samples: int, seed: int,
                                      want_path: bool = True, want_usage: bool = False):
        """n_samples (1..64) draws from the posterior over paths of every read over its lists, P(path | read, model,
        lists): the forward sums as the filter and one random walk back per sample (include/phmm_amd_sample.h, which
        writes out the sums, the random stream and the draw rule)
        -> (logp[R], path_logp[R, S], path[S, total_bases, stride] | None, counts[R, S, 4], usage[S, n_nodes] | None).
        logp[r] = ln Z, the forward total of the read over its lists as sets (-inf: no path); path_logp = ln P of each
        sampled path; plane s of path is sample s of every read in the rows of run_with_mapping_best_path, so
        path_states(mappings, read, path[s]) works on it; counts = matches, mismatches, insertions, deletions of each
        sample; usage[s, v] = the Match, Ins and Del states of all reads on node v in sample s, one draw of what the
        node frequencies are the expectation of.  A read's samples depend on seed, its index and s alone."""
        R, S = len(reads), int(n_samples)
        stride = int(self.param.n_max_gaps) + 2
        lp = np.empty(R)
        plp = np.empty((R, max(S, 0)))
        counts = np.empty((R, max(S, 0), 4), dtype=np.uint32)
        path = np.empty((max(S, 0), reads.total_bases(), stride), dtype=np.uint32) if want_path else None
        usage = np.empty((max(S, 0), self.n_nodes), dtype=np.uint32) if want_usage else None
        _ffi.check(_ffi.lib().phmm_run_with_mapping_sample_paths(
            self._h, reads._h, mappings._h, S, int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(lp), _ptr(plp) if plp.size else None,
            _ptr(path) if want_path and path.size else None, _ptr(counts) if counts.size else None,
            _ptr(usage) if want_usage and usage.size else None))
        return lp, plp, path, counts, usage

    def run_with_mapping_alignments(self, reads: ReadCollection, mappings: Mappings, n_samples: int = 0, seed: int = 0):
        """The best path (n_samples = 0) or n_samples (1..64) sampled paths of every read over its lists as alignment
        records, built on the device from rows that never leave it (include/phmm_amd_align.h)
        -> (logp[R], path_logp[R, S] | None, counts[R, S', 4], Alignments), S' = max(n_samples, 1).
        logp is the best ln P or ln Z; path_logp the ln P of each sample (None for the best path); counts the =, X, I, D
        totals of each alignment; the walks are those run_with_mapping_best_path / run_with_mapping_sample_paths return
        for the same arguments."""
        from . import _ffi_align
        R, S = len(reads), int(n_samples)
        planes = max(S, 1)
        lp = np.empty(R)
        plp = np.empty((R, S)) if S else None
        counts = np.empty((R, planes, 4), dtype=np.uint32)
        h = C.c_void_p()
        _ffi.check(_ffi_align.lib().phmm_run_with_mapping_alignments(
            self._h, reads._h, mappings._h, S, int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(lp),
            _ptr(plp) if S and plp.size else None, _ptr(counts) if counts.size else None, C.byref(h)))
        return lp, plp, counts, Alignments(h, R, S)

    def run_with_mapping_read_usage(self, reads: ReadCollection, mappings: Mappings, groups=None, want_totals: bool = True):
        """Per read, how often the read used every node by state over its lists (include/phmm_amd_usage.h):
        PHMMOutput::to_state_probs() / to_node_freqs() of every read, as a sparse read-by-key matrix reduced on the
        device from the values of run_with_mapping_states, which never leave it -> (logp_forward[R], ReadUsage).
        groups = (group_off, group_nodes) as for Likelihood.set_groups: the key of a node is its group, and the entries
        of a node in no group are left out; None: the key of a node is the node.  want_totals: ReadUsage.totals[K, 3],
        the column sums over all reads.  Every sum runs in a fixed order, so a read's row depends on the model, the read
        and its lists alone."""
        from . import _ffi_usage
        R = len(reads)
        n_groups, g_off, g_nodes = 0, None, None
        if groups is not None:
            g_off = np.ascontiguousarray(groups[0], dtype=np.uint64).reshape(-1)
            g_nodes = np.ascontiguousarray(groups[1], dtype=np.uint32).reshape(-1)
            n_groups = g_off.shape[0] - 1
            if n_groups < 1:
                raise ValueError("groups: group_off needs at least two entries")
        K = n_groups if n_groups else self.n_nodes
        lf = np.empty(R)
        totals = np.zeros((K, 3)) if want_totals else None
        h = C.c_void_p()
        _ffi.check(_ffi_usage.lib().phmm_run_with_mapping_read_usage(
            self._h, reads._h, mappings._h, n_groups, _ptr(g_off), _ptr(g_nodes) if n_groups and g_nodes.size else None,
            _ptr(lf), _ptr(totals) if want_totals and R else None, C.byref(h)))
        return lf, ReadUsage(h, R, K, totals)

    def run_with_mapping_pileup(self, reads: ReadCollection, mappings: Mappings, want_rows: bool = True,
                                want_totals: bool = True):
        """Per node, which bases the reads showed there, by state, over their lists (include/phmm_amd_pileup.h): the
        values of run_with_mapping_states, which never leave the device, reduced there under the key 4 * node + base
        code of the read base at the entry's position (A 0, C 1, G 2, T 3) -> (logp_forward[R], Pileup).
        want_rows: the per-read rows, keyed by (node, base); want_totals: Pileup.totals[N, 9], per node the Match mass by
        read base, the Ins mass by read base and the Del mass over all reads.  A read holding a byte other than A C G T
        is refused.  Every sum runs in a fixed order, so a read's row depends on the model, the read and its lists
        alone."""
        from . import _ffi_pileup
        R, N = len(reads), self.n_nodes
        lf = np.empty(R)
        totals = np.zeros((N, 9)) if want_totals else None
        h = C.c_void_p()
        _ffi.check(_ffi_pileup.lib().phmm_run_with_mapping_pileup(
            self._h, reads._h, mappings._h, _ptr(lf), _ptr(totals) if want_totals and R else None,
            C.byref(h) if want_rows else None))
        return lf, Pileup(h if want_rows else None, R, N, totals)

    def run_with_mapping_read_edges(self, reads: ReadCollection, mappings: Mappings, edge_key=None, init_key=None,
                                    n_keys: int = 0, want_totals: bool = True):
        """Per read, which transitions of the graph the read crossed over its lists and how often
        (include/phmm_amd_edges.h): PHMMOutput::to_edge_and_init_freqs() of every read, as a sparse read-by-key matrix
        reduced on the device from the records of the list pass of run_with_mapping_edge_freqs, which never leave it
        -> (logp_forward[R], ReadEdges).
        n_keys = 0: the key of edge e is e and that of Begin -> v is E + v.  Otherwise edge_key[E] / init_key[N] give
        the key (< n_keys) of every edge / Begin transition, PHMM_NO_KEY (0xffffffff) leaving a term out and None
        leaving the whole kind out; edges on one key add (link_keys builds the map of unitig junctions).
        want_totals: ReadEdges.totals[K], the column sums over all reads.  Every sum runs in a fixed order, so a read's
        row depends on the model, the read, its lists and the knobs alone."""
        from . import _ffi_edges
        R, n_keys = len(reads), int(n_keys)
        ek = ik = None
        if n_keys:
            if edge_key is not None:
                ek = np.ascontiguousarray(edge_key, dtype=np.uint32).reshape(-1)
                if ek.shape[0] != self.n_edges:
                    raise ValueError("edge_key needs one entry per edge")
            if init_key is not None:
                ik = np.ascontiguousarray(init_key, dtype=np.uint32).reshape(-1)
                if ik.shape[0] != self.n_nodes:
                    raise ValueError("init_key needs one entry per node")
        elif edge_key is not None or init_key is not None:
            raise ValueError("edge_key / init_key need n_keys > 0")
        K = n_keys if n_keys else self.n_edges + self.n_nodes
        lf, end_terms = np.empty(R), np.empty((R, 2))
        totals = np.zeros(K) if want_totals else None
        h = C.c_void_p()
        _ffi.check(_ffi_edges.lib().phmm_run_with_mapping_read_edges(
            self._h, reads._h, mappings._h, n_keys, _ptr(ek) if ek is not None and ek.size else None,
            _ptr(ik) if ik is not None else None, _ptr(lf), _ptr(end_terms) if R else None,
            _ptr(totals) if want_totals and R else None, C.byref(h)))
        return lf, ReadEdges(h, R, K, totals, end_terms, None if n_keys else self.n_edges)

    _GEN_KINDS = {"state_count": 0, "endable": 1, "emit_count": 2}

    def sample_reads_raw(self, first_index: int, n_walks: int, length: int, kind: str = "state_count", start_nodes=None,
                         seed: int = 0, want_history: bool = False, want_usage: bool = False):
        """phmm_sample_reads (include/phmm_amd_generate.h) for the walks first_index .. first_index + n_walks - 1
        -> (bases[n_walks, length + 1] uint8 padded with 0, len[n_walks], flags[n_walks], history[n_walks, cap] | None,
        history_len[n_walks] | None, usage[n_nodes] | None); cap = length + 1, or 8 * length + 65 under emit_count, so
        no history is truncated."""
        n, length = int(n_walks), int(length)
        sn = None if start_nodes is None else np.ascontiguousarray(start_nodes, dtype=np.uint32).reshape(-1)
        bases = np.empty((n, length + 1), dtype=np.uint8)
        ln, fl = np.empty(n, dtype=np.uint32), np.empty(n, dtype=np.uint32)
        cap = (8 * length + 65 if kind == "emit_count" else length + 1) if want_history else 0
        hist = np.empty((n, cap), dtype=np.uint32) if want_history else None
        hl = np.empty(n, dtype=np.uint32) if want_history else None
        usage = np.empty(self.n_nodes, dtype=np.uint32) if want_usage else None
        _ffi.check(_ffi.lib().phmm_sample_reads(
            self._h, int(first_index), n, length, self._GEN_KINDS[kind], _ptr(sn), 0 if sn is None else sn.size,
            int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(bases) if n else None, _ptr(ln) if n else None, _ptr(fl) if n else None,
            _ptr(hist) if want_history and n else None, cap, _ptr(hl) if want_history and n else None, _ptr(usage)))
        return bases, ln, fl, hist, hl, usage

    def sample_reads(self, length: int, kind: str = "state_count", n_reads: Optional[int] = None,
                     total_bases: Optional[int] = None, start_nodes=None, seed: int = 0, want_history: bool = False,
                     batch: int = 4096):
        """Reads drawn from the model on the device: sample_by_profile (sample.rs:198-235) over phmm_sample_reads
        (include/phmm_amd_generate.h, which writes out the walk, the random stream and the draw rule)
        -> (ReadCollection, info).
        kind: 'state_count', 'endable' or 'emit_count' (ReadLength::StateCount / Endable / EmitCount of `length`);
        start_nodes: StartPoints::Custom (None: the walks start in MatchBegin).  The walks 0, 1, 2, .. of `seed` are
        taken in index order, `batch` per call; a walk without bases is dropped, and under 'emit_count' a walk whose
        length is not `length` (the reference's retry loop).  Exactly one of n_reads (ReadAmount::Count) and total_bases
        (ReadAmount::TotalBases: walks are accepted until their bases reach the total, the read that crosses it kept)
        ends the loop.  info = dict(walk_index[R], flags[R] (PHMM_GEN_* bits), n_walks = the walks consumed, the last
        accepted one included, and with want_history history = [uint32 words per read]: (node << 2) | 0 Match / 1 Ins /
        2 Del, PATH_INS_BEGIN, or 0xfffffffc for End).  The result does not depend on batch."""
        if (n_reads is None) == (total_bases is None):
            raise ValueError("give exactly one of n_reads and total_bases")
        if kind not in self._GEN_KINDS:
            raise ValueError("kind is 'state_count', 'endable' or 'emit_count'")
        batch = max(1, int(batch))
        reads: List[bytes] = []
        index: List[int] = []
        flags: List[int] = []
        history: List[np.ndarray] = []
        got, first, consumed = 0, 0, 0

        def more():
            return len(reads) < n_reads if n_reads is not None else got < total_bases
        while more():
            if first - consumed > (1 << 20):
                raise RuntimeError("sample_reads: no walk accepted among the last 2^20")
            bases, ln, fl, hist, hl, _ = self.sample_reads_raw(first, batch, length, kind, start_nodes, seed, want_history)
            for w in range(batch):
                n = int(ln[w])
                if n == 0 or (kind == "emit_count" and n != length):
                    continue
                reads.append(bases[w, :n].tobytes())
                index.append(first + w)
                flags.append(int(fl[w]))
                if want_history:
                    history.append(hist[w, :int(hl[w])].copy())
                got += n
                consumed = first + w + 1
                if not more():
                    break
            first += batch
        info = dict(walk_index=np.array(index, dtype=np.uint64), flags=np.array(flags, dtype=np.uint32), n_walks=consumed)
        if want_history:
            info["history"] = history
        return ReadCollection(reads), info

    def q_score_exact(self, edge_freqs: np.ndarray, init_freqs: np.ndarray):
        """q_score_exact (src/hmmv2/q.rs:66-96) -> (init, trans, prior); QScore::total() is their sum."""
        ef = np.ascontiguousarray(edge_freqs, dtype=np.float64)
        nf = np.ascontiguousarray(init_freqs, dtype=np.float64)
        if ef.size < self.n_edges or nf.size < self.n_nodes:
            raise ValueError("edge_freqs / init_freqs shorter than the model")
        q = np.empty(3)
        _ffi.check(_ffi.lib().phmm_q_score_exact(self._h, _ptr(ef) if self.n_edges else None, _ptr(nf), _ptr(q)))
        return float(q[0]), float(q[1]), float(q[2])

    def to_full_prob_reads_copy_nums(self, reads: ReadCollection, mappings: Mappings, copy_nums: np.ndarray,
                                     min_copy_num: int = 0):
        """The same loop with candidates given as copy-number vectors [C,N] (what the sampler varies,
        posterior.rs:483-515); init / trans are derived on the device as SeqGraph::to_phmm does
        (seq_graph.rs:160-209)."""
        cn = np.ascontiguousarray(copy_nums, dtype=np.uint32)
        Cn = cn.shape[0]
        lp = np.empty((Cn, len(reads)))
        tot = np.empty(Cn)
        _ffi.check(_ffi.lib().phmm_full_prob_reads_copy_nums(self._h, reads._h, mappings._h, Cn, _ptr(cn),
                                                             int(min_copy_num), _ptr(lp), _ptr(tot)))
        return tot, lp

    def to_full_prob_reads_copy_num_changes(self, reads: ReadCollection, mappings: Mappings, base: np.ndarray,
                                            changes, min_copy_num: int = 0, out_logp=None):
        """The loop of sample_posterior_once (posterior.rs:483-515) with each candidate given as changes to the base
        copy-number vector: changes = (off[C+1], node, cn), candidate c = base with cn[node[j]] = cn[j] for j in
        [off[c], off[c+1]) (see copy_num_changes).  Only the reads whose lists meet a changed node or one of its
        parents are run again; the others get ln P_base + ln(T_base / T_c).  Same values as
        to_full_prob_reads_copy_nums on the materialised vectors -> (totals[C], per_read[C,R], n_rescored[C])."""
        b = np.ascontiguousarray(base, dtype=np.uint32)
        off, node, cn = changes
        off = np.ascontiguousarray(off, dtype=np.uint64)
        node = np.ascontiguousarray(node, dtype=np.uint32)
        cn = np.ascontiguousarray(cn, dtype=np.uint32)
        Cn = off.size - 1
        lp = np.empty((Cn, len(reads))) if out_logp is None else out_logp
        tot = np.empty(Cn)
        nr = np.empty(Cn, dtype=np.uint64)
        _ffi.check(_ffi.lib().phmm_full_prob_reads_copy_num_changes(
            self._h, reads._h, mappings._h if mappings else None, _ptr(b), int(min_copy_num), Cn, _ptr(off),
            _ptr(node), _ptr(cn), _ptr(lp), _ptr(tot), _ptr(nr)))
        return tot, lp, nr

    def likelihood(self, reads: ReadCollection, mappings: Mappings, copy_nums: np.ndarray,
                   min_copy_num: int = 0) -> "Likelihood":
        """MultiDbg::to_likelihood (posterior.rs:247-255) as a device-resident state for the greedy search of
        sample_posterior (posterior.rs:314-417): see Likelihood."""
        return Likelihood(self, reads, mappings, copy_nums, min_copy_num)

    def generate_mappings(self, reads: ReadCollection, mappings: Optional[Mappings] = None,
                          use_max_ratio: bool = True, out_node_freq=None):
        """PHMMModel::generate_mappings (hint.rs:193-220) -> (Mappings, node_freq[N])."""
        h = C.c_void_p()
        nf = np.empty(self.n_nodes) if out_node_freq is None else out_node_freq
        _ffi.check(_ffi.lib().phmm_generate_mappings(self._h, reads._h, mappings._h if mappings else None,
                                                     int(use_max_ratio), C.byref(h), _ptr(nf)))
        return Mappings(h, reads), nf


def copy_num_changes(base: np.ndarray, candidates: np.ndarray):
    """Candidates [C,N] as changes to the base copy-number vector [N] -> CSR (off[C+1] uint64, node uint32,
    cn uint32): the nodes where candidate c differs from the base, ascending, with their new copy numbers."""
    b = np.asarray(base, dtype=np.uint32).reshape(-1)
    cands = np.asarray(candidates, dtype=np.uint32).reshape(-1, b.size)
    ci, node = np.nonzero(cands != b[None, :])
    off = np.zeros(cands.shape[0] + 1, dtype=np.uint64)
    np.cumsum(np.bincount(ci, minlength=cands.shape[0]), out=off[1:])
    return off, node.astype(np.uint32), cands[ci, node].astype(np.uint32)


class Likelihood:
    """The sampler's state at one k, on the device: the current copy-number vector and every read's ln P under it,
    for the whole greedy search of sample_posterior (multi_dbg/posterior.rs:314-417).  score_changes is the loop of
    sample_posterior_once over the neighbours of the current vector (posterior.rs:470-528) without a base pass; move
    is the step to the best neighbour or to the union of several independent moves (posterior.rs:532-600), rescoring
    only the reads the move touches.  Borrows model, reads and mappings (kept alive here)."""

    def __init__(self, model: "PHMMModel", reads: ReadCollection, mappings: Mappings, copy_nums: np.ndarray,
                 min_copy_num: int = 0):
        self.model, self.reads, self.mappings = model, reads, mappings
        cn = np.ascontiguousarray(copy_nums, dtype=np.uint32).reshape(-1)
        if cn.size != model.n_nodes:
            raise ValueError("copy_nums must have one entry per node")
        h = C.c_void_p()
        _ffi.check(_ffi.lib().phmm_likelihood_create(model._h, reads._h, mappings._h if mappings else None, _ptr(cn),
                                                     int(min_copy_num), C.byref(h)))
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            _ffi.lib().phmm_likelihood_destroy(self._h)
            self._h = None

    def score_changes(self, changes, out_logp=None, per_read: bool = True):
        """Candidates as changes to the CURRENT vector, changes = (off[C+1], node, cn) as copy_num_changes builds them
        (sample_posterior_once, posterior.rs:470-528) -> (totals[C], per_read[C,R] or None, n_rescored[C]).
        per_read=False forms no [C,R] matrix anywhere."""
        off, node, cn = changes
        off = np.ascontiguousarray(off, dtype=np.uint64)
        node = np.ascontiguousarray(node, dtype=np.uint32)
        cn = np.ascontiguousarray(cn, dtype=np.uint32)
        Cn = off.size - 1
        lp = out_logp if out_logp is not None else (np.empty((Cn, len(self.reads))) if per_read else None)
        tot = np.empty(Cn)
        nr = np.empty(Cn, dtype=np.uint64)
        _ffi.check(_ffi.lib().phmm_likelihood_score_changes(self._h, Cn, _ptr(off), _ptr(node), _ptr(cn), _ptr(lp),
                                                            _ptr(tot), _ptr(nr)))
        return tot, lp, nr

    def move(self, nodes, copy_nums):
        """current[nodes] = copy_nums: one candidate of the last batch or the union of several (posterior.rs:532-600)
        -> (ln P(R | new vector), reads rescored)."""
        node = np.ascontiguousarray(nodes, dtype=np.uint32).reshape(-1)
        cn = np.ascontiguousarray(copy_nums, dtype=np.uint32).reshape(-1)
        if node.size != cn.size:
            raise ValueError("nodes and copy_nums differ in length")
        tot = np.empty(1)
        nr = np.empty(1, dtype=np.uint64)
        _ffi.check(_ffi.lib().phmm_likelihood_move(self._h, node.size, _ptr(node), _ptr(cn), _ptr(tot), _ptr(nr)))
        return float(tot[0]), int(nr[0])

    def current(self):
        """-> (copy_nums[N], per-read ln P [R], their sum) under the current vector."""
        cn = np.empty(self.model.n_nodes, dtype=np.uint32)
        lp = np.empty(len(self.reads))
        tot = np.zeros(1)
        _ffi.check(_ffi.lib().phmm_likelihood_current(self._h, _ptr(cn), _ptr(lp), _ptr(tot)))
        return cn, lp, float(tot[0])

    def refresh(self) -> None:
        """Rescore the current vector in full (after PHMMModel.set_params)."""
        _ffi.check(_ffi.lib().phmm_likelihood_refresh(self._h))

    # ---- the same calls in the sampler's own units: node groups = the k-mers of one compact edge
    def set_groups(self, group_off, group_nodes) -> None:
        """Groups of nodes the sampler changes together: group g = group_nodes[group_off[g]:group_off[g+1]], the
        k-mers of one compact edge (MultiDbg::edges_in_full; set_copy_nums writes one compact edge's copy number
        into every k-mer of its unitig, multi_dbg.rs:1041-1052).  Disjoint; the current vector must be constant
        within each.  Replaces earlier groups; an empty group_off removes them.  graph.unitig_groups builds them for
        a SeqGraph."""
        off = np.ascontiguousarray(group_off, dtype=np.uint64).reshape(-1)
        nodes = np.ascontiguousarray(group_nodes, dtype=np.uint32).reshape(-1)
        n_groups = max(off.size - 1, 0)
        if n_groups and int(off[-1]) != nodes.size:
            raise ValueError("group_off[-1] must be len(group_nodes)")
        _ffi.check(_ffi.lib().phmm_likelihood_set_groups(self._h, n_groups, _ptr(off), _ptr(nodes)))
        self.n_groups = n_groups

    def score_group_changes(self, changes, out_logp=None, per_read: bool = True):
        """score_changes with changes = (off[C+1], group, cn) in group units: the neighbours of sample_posterior_once
        (posterior.rs:470-528) as UpdateInfo::cycle() states them, +1 / -1 on compact edges -- bit for bit what
        score_changes returns for the lists expanded to nodes -> (totals[C], per_read[C,R] or None, n_rescored[C])."""
        off, group, cn = changes
        off = np.ascontiguousarray(off, dtype=np.uint64)
        group = np.ascontiguousarray(group, dtype=np.uint32)
        cn = np.ascontiguousarray(cn, dtype=np.uint32)
        Cn = off.size - 1
        lp = out_logp if out_logp is not None else (np.empty((Cn, len(self.reads))) if per_read else None)
        tot = np.empty(Cn)
        nr = np.empty(Cn, dtype=np.uint64)
        _ffi.check(_ffi.lib().phmm_likelihood_score_group_changes(self._h, Cn, _ptr(off), _ptr(group), _ptr(cn),
                                                                  _ptr(lp), _ptr(tot), _ptr(nr)))
        return tot, lp, nr

    def move_groups(self, groups, copy_nums):
        """move in group units: every node of groups[j] takes copy_nums[j] (posterior.rs:532-600; set_copy_nums,
        multi_dbg.rs:1041-1052) -> (ln P(R | new vector), reads rescored)."""
        group = np.ascontiguousarray(groups, dtype=np.uint32).reshape(-1)
        cn = np.ascontiguousarray(copy_nums, dtype=np.uint32).reshape(-1)
        if group.size != cn.size:
            raise ValueError("groups and copy_nums differ in length")
        tot = np.empty(1)
        nr = np.empty(1, dtype=np.uint64)
        _ffi.check(_ffi.lib().phmm_likelihood_move_groups(self._h, group.size, _ptr(group), _ptr(cn), _ptr(tot),
                                                          _ptr(nr)))
        return float(tot[0]), int(nr[0])

    def current_groups(self) -> np.ndarray:
        """The current vector in group units, as get_copy_nums returns it over compact edges (PosteriorSample.copy_nums,
        posterior.rs:314-417; multi_dbg.rs:1041-1052 is its inverse) -> uint32[G], _ffi.PHMM_GROUP_MIXED for a group
        a node-form move has split."""
        out = np.empty(getattr(self, "n_groups", 0), dtype=np.uint32)
        _ffi.check(_ffi.lib().phmm_likelihood_current_groups(self._h, _ptr(out)))
        return out


class PHMMOutput:
    """PHMMOutput (src/hmmv2/table.rs:450-517) of one dense run."""

    def __init__(self, model: PHMMModel, read: bytes, forward: DenseTables, backward: DenseTables):
        self.model, self.read, self.forward, self.backward = model, read, forward, backward

    def to_full_prob_forward(self) -> float:
        return float(self.forward.e[-1])

    def to_full_prob_backward(self) -> float:
        return float(self.backward.mb[0])

    def to_emit_probs(self, merged_index: int):
        """table.rs:500-505 with the merged indexing of table.rs:414-434 (log values)."""
        L = len(self.forward)
        p = self.to_full_prob_forward()
        n = self.model.n_nodes
        ninf = np.full(n, -np.inf)
        if merged_index == 0:
            fm, fi, fd = ninf, ninf, ninf
        else:
            fm, fi, fd = (self.forward.m[merged_index - 1], self.forward.i[merged_index - 1],
                          self.forward.d[merged_index - 1])
        if merged_index >= L:
            pe = np.full(n, self.model.param.p_end)
            bm, bi, bd = pe, pe, pe
        else:
            bm, bi, bd = self.backward.m[merged_index], self.backward.i[merged_index], self.backward.d[merged_index]
        return fm + bm - p, fi + bi - p, fd + bd - p

    def to_node_freqs(self) -> np.ndarray:
        """freq.rs:245-255 through the device path (single-read run_dense)."""
        rc = ReadCollection([self.read])
        _, _, nf = self.model.run_dense(rc, True, True)
        return nf
