"""A parameter set whose fifteen probabilities all differ, and the small seeded fixtures the parity tests run it on.

Every set PHMMParams.new / uniform makes has p_MI = p_MD = p_ID = p_DI, p_II = p_DD, p_IM = p_DM, p_random = ln 1/4 and
p_match = ln(1 - p_mismatch); so has every other parameter set of the suite.  Two tied fields exchanged in a kernel's
hand-made copy of the struct, a hard-coded 0.25 or a 1 - mismatch computed on the device change nothing under those.
DISTINCT ties nothing: the rows out of Match, Ins and Del still sum to 1 with p_end.

tests/test_distinct_params_cpu.py asserts what is said of the fixtures here and that every exchange moves every output
of the oracle by at least 100 times the bar tests/test_gpu_distinct_params.py holds that output to.
"""
import ctypes as C
import functools
import math

import numpy as np

import dbgphmm_amd as D
from best_path_ref import pad_lists
from repeat_cases import dataset

LINEAR = dict(p_mismatch=0.03, p_match=0.95, p_random=0.21, p_gap_open=0.011, p_gap_ext=0.13, p_end=0.002,
              p_MI=0.020, p_MD=0.045, p_MM=0.933,
              p_II=0.09, p_ID=0.031, p_IM=0.877,
              p_DI=0.012, p_DD=0.06, p_DM=0.926)
DISTINCT = {k: math.log(v) for k, v in LINEAR.items()}
FIELDS = tuple(LINEAR)

# the ties of new() / uniform(), as exchanges and de-tunings that a tied set cannot see
SWAPS = (("p_MI", "p_MD"), ("p_ID", "p_DI"), ("p_II", "p_DD"), ("p_IM", "p_DM"))
DETUNED = {"p_random = 1/4": dict(p_random=math.log(0.25)),
           "p_match = 1 - p_mismatch": dict(p_match=math.log(1.0 - LINEAR["p_mismatch"]))}
PADS = (64, 65, 400)


def params(k, gaps=4, **over):
    return D.PHMMParams.uniform(0.01).with_(n_warmup=k, n_max_gaps=gaps, **{**DISTINCT, **over})


def swapped(a, b):
    """the overrides that exchange fields a and b of DISTINCT (for params(k, **swapped(a, b)))"""
    return {a: DISTINCT[b], b: DISTINCT[a]}


def changes():
    """name -> overrides: the four exchanges and the two de-tunings"""
    out = {f"{a} / {b} swapped": swapped(a, b) for a, b in SWAPS}
    out.update(DETUNED)
    return out


def with_param(arrays, param):
    """the same model under other parameters (the arrays do not depend on them: graph.py takes init and transition
    probabilities from the copy numbers alone)"""
    return D.PHMMArrays(param, arrays.emission, arrays.init_logp, arrays.edge_src, arrays.edge_dst, arrays.trans_logp,
                        arrays.is_emittable)


def offsets(reads):
    off = np.zeros(len(reads) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    return off


def oracle_lists(arrays, reads):
    from oracle import oracle as O
    O.build()
    (po, nd, lp), _ = O.Model(arrays).generate_mappings(reads, None, True, n_threads=8)
    return po, nd, lp


@functools.lru_cache(maxsize=None)
def dbg():
    """an 800-base diploid genome at k = 24 (1118 nodes), eight reads of 60 to 120 bases -> dict(arrays, sg, reads)"""
    hap = D.random_genome(800, 7)
    sg = D.dbg_from_haplotypes([hap, D.diverge(hap, 0.02, 8)], 24)
    arrays = D.vectorised_to_phmm(sg, params(24), 0)
    reads = [r for r in D.sample_reads(arrays, 10 ** 9, 120, seed=9, max_reads=16) if len(r) >= 60][:8]
    assert len(reads) == 8
    return dict(arrays=arrays, sg=sg, reads=reads)


def with_indels(read, at_ins=90, at_del=140):
    """the read with two bases inserted at at_ins (each the successor of the base it stands before, then the one after)
    and the two bases at at_del taken out"""
    x = bytearray(read)
    del x[at_del:at_del + 2]
    x[at_ins:at_ins] = [b"ACGT"[(b"ACGT".index(bytes([x[at_ins + j]])) + 1 + j) % 4] for j in range(2)]
    return bytes(x)


@functools.lru_cache(maxsize=None)
def u20():
    """the 20 bp x 50 tandem repeat at k = 40 (555 nodes), six reads cut to 200 bases -> dict(arrays, sg, reads).  The
    reads come from uniform(0.001) and are nearly free of errors; on the last one the effects of p_II and p_DD cancel
    (exchanging the two moves its ln P by 7e-6), so it carries a two-base insertion and a two-base deletion."""
    arrays, reads, sg, _ = dataset("u20", 40, max_reads=6)
    reads = [r[:200] for r in reads]
    reads[5] = with_indels(reads[5])
    return dict(arrays=with_param(arrays, params(40)), sg=sg, reads=reads)


@functools.lru_cache(maxsize=None)
def lists_of(which):
    """the oracle's own lists of a fixture ("dbg" / "u20") -> (pos_off, nodes, logp)"""
    f = dbg() if which == "dbg" else u20()
    return oracle_lists(f["arrays"], f["reads"])


@functools.lru_cache(maxsize=None)
def padded(which, width):
    """lists_of(which) padded to `width` at two of every three positions -> (pos_off, nodes)"""
    f = dbg() if which == "dbg" else u20()
    po, nd, _ = lists_of(which)
    return pad_lists(po, nd, f["reads"], f["arrays"].n_nodes, width)


CUT_AT, DEEP_CUT_AT = 50, 170


def _cut(read, po, nd, at):
    """dbg() with the best node of base `at` of `read` (lists po, nd) at copy number 0"""
    f = dbg()
    cn = f["sg"].copy_num.copy()
    cn[int(nd[int(po[at])])] = 0
    sg = D.SeqGraph(cn, f["sg"].base, f["sg"].edge_src, f["sg"].edge_dst, None)
    with np.errstate(divide="ignore"):
        arrays = D.vectorised_to_phmm(sg, params(24), 0)
    return dict(arrays=arrays, sg=sg, reads=[read], lists=(po, nd))


@functools.lru_cache(maxsize=None)
def cut_read():
    """dbg() with the best node of base 50 of read 0 at copy number 0: the read's path is cut there and the InsBegin chain
    (p_random, p_II, p_IM, p_ID) carries it -> dict(arrays, sg, reads: [read 0], lists: its lists on the uncut model).
    The chain stands 223 bits under the column before it, which the scaled kernels still hold: this read stays with
    them (the hinted kernels hand a read to the exact one when a column drops by more than 512 bits)."""
    f = dbg()
    po, nd, _ = lists_of("dbg")
    n = len(f["reads"][0])
    return _cut(f["reads"][0], po[:n + 1].copy(), nd[:int(po[n])].copy(), CUT_AT)


@functools.lru_cache(maxsize=None)
def deep_cut_read():
    """the same with a read long enough to reach the exact hinted kernel: 200 bases of the first haplotype, cut at base
    170 (no read of dbg() is longer than 118 bases, and a cut at the end of one drops by 524 bits at most)"""
    read = bytes(D.random_genome(800, 7))[100:300]
    po, nd, _ = oracle_lists(dbg()["arrays"], [read])
    return _cut(read, po, nd, DEEP_CUT_AT)


def chimera():
    """the first 60 bases of read 0 and the first 100 of read 1 of dbg(), joined.  The dense certificate
    (exact_dense.hip: certify_dense) sends a read to the exact path when max F of a column times max B of the next
    exceeds P by about 613 nats; here it is 25, so this read stays on the scaled kernels."""
    r = dbg()["reads"]
    return r[0][:60] + r[1][:100]


@functools.lru_cache(maxsize=None)
def deep_chimera():
    """a chimera that does take the exact dense path -> (arrays, read): dbg()'s construction on a genome of 1700 bases
    (2260 nodes), bases 0..459 and 900..1359 of its first haplotype joined (783 nats by the same measure; the 800 bases
    of dbg() give 504 at most)"""
    hap = D.random_genome(1700, 7)
    sg = D.dbg_from_haplotypes([hap, D.diverge(hap, 0.02, 8)], 24)
    hb = bytes(hap)
    return D.vectorised_to_phmm(sg, params(24), 0), hb[:460] + hb[900:1360]


# the walks compared word for word; a seed whose walks fail the margin condition of the CPU test is replaced here
SAMPLE_SEED = 21                               # run_with_mapping_sample_paths, 4 samples per read
GEN_SEED, GEN_WALKS, GEN_LENGTH = 31, 64, 100  # phmm_sample_reads on dbg()'s model


def walk_case(width):
    """dbg() on its generated lists (width None) or on the padded ones -> (arrays, reads, pos_off, nodes); at 400 the
    first three reads, which keeps the Python restatements of the walks near a second"""
    f = dbg()
    po, nd = lists_of("dbg")[:2] if width is None else padded("dbg", width)
    reads = f["reads"]
    if width == 400:
        reads = reads[:3]
        n = sum(len(r) for r in reads)
        po, nd = po[:n + 1], nd[:int(po[n])]
    return f["arrays"], reads, po, nd


def set_tie_rule(oracle, eps, mode):
    L = oracle.lib()
    L.orc_set_tie_rule.argtypes = [C.c_double, C.c_int]
    L.orc_set_tie_rule(eps, mode)
