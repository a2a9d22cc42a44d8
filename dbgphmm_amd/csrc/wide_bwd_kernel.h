// The 400-slot class of backward_by_forward + to_mapping_by_score_ratio on ONE BLOCK of 448 threads per read
// (7 waves; thread = slot), the counterpart of wide_fwd_kernel.h.
//
// sparse_backward_kernel<400> (mapping_flow.hip) walks a read position with one wave: the forward record's totals are
// sorted (400 x 400 comparisons on 64 lanes), the column B.tables[pos] is computed over the record's nodes (backward.rs:
// 122-129, 216-261: bd0 + n_max_gaps x bdt restricted to the list, bm, bi), the posterior S = F (.) B / P
// (table.rs:500-505) is cut at the score ratio and sorted again (hint.rs:135-142).  Every one of these passes is a loop
// over the slots: seven iterations of a wave on a 400-node column, one here.  Same statements, same per-node summation
// order (the packed records keep the CSR order of a node's children); a slot's adjacency record and the slots of its
// in-list children are found once per position and stay in the thread's registers through the Del sweeps.
// Score-ratio lists only (topk == 0), packed records: the host keeps the generic kernel otherwise.
//
// Two flavours behind a template flag, as the EDGES flag of sparse_backward_kernel (what belongs to the other flavour is
// discarded at compile time: the adaptive flavour's instructions are those it had before the flag):
//   * wide_backward_kernel<false>: backward_by_forward of the adaptive flow -- the node list of a column is the forward
//     record's elements by total, bursts and hand-offs between the capacity classes, the dense hand-over at s0;
//   * wide_backward_kernel<true>: backward_with_mapping (backward.rs:59-93, the list mode of sparse_backward_kernel,
//     mapping_flow.hip) -- the node list of position pos is mapping.nodes(pos), read from a.list_nodes into sh.list in
//     the place of the sort.  The walk goes down to position 0, whose column has no forward record and emits nothing:
//     only its MatchBegin, summed over the list at that position alone, leaves the kernel as a.logb (the read's
//     backward total).  No hand-off, no burst, no dense hand-over; a.stop / a.err as the one-wave list kernel leaves
//     them (a missing forward record or a list beyond the block: SP_ERR_CAPACITY).
//   * wide_backward_kernel<true, true>: the transition-posterior form of the list flavour (sparse_backward_kernel<CAP,
//     true>, mapping_flow.hip): the same columns, and where the list flavour cuts the posterior into a mapping list this
//     one writes the edge and Begin terms of merged index pos (emit_edge_terms / emit_begin_terms, thread = slot) into
//     the record of position pos.  A thread's terms go behind those of the threads before it (a block scan of the
//     counts of non-zero terms): slot-major, child-minor, the order rec_append gives the one-wave kernel's chunks of 64.
//   * wide_backward_kernel<true, false, BS, true>: the state-posterior form (sparse_backward_kernel<CAP, false, true>):
//     the same columns, and in the place of the mapping list the three logs of to_emit_probs by state for every entry
//     of the INPUT list of position pos-1, thread = slot of that list, plus the head of to_states() of the position: a
//     wave reduction over (value, kind, slot) and one pair per wave through sh.red / sh.wsum (wb_states).  No sort.
// The block has two sizes (BS): 448 threads for lists of up to 400 nodes, and, for the list flavours, 128 threads (two
// waves, a third of the LDS) for reads whose longest list holds at most 128 nodes.  Both run the same per-slot
// expressions, the same wave-0 sums (lane j adds the slots j, j + 64, ...), the same sorting network on the same padded
// size and the same scan offsets: the small block gives the bits of the large one.
// Every exit from the walk is taken by the whole block: it is decided from values every thread holds alike (a record
// offset or a list size read from memory, an allocation published through LDS).
#pragma once

#include "block_sort.h"
#include "sparse_dyn.h"

namespace phmm {

static constexpr int WBK_T = 448;
static constexpr int WBK_T_SMALL = 128;  // the list flavours' block for reads with lists of at most 128 nodes
static constexpr int WBK_CAP = PHMM_MAX_ACTIVE_NODES;

template <int BS> struct WBColT {
    static constexpr int HASH = BS > 128 ? 1024 : 512, HASH_SHIFT = BS > 128 ? 22 : 23;
    double m[BS], i[BS], d[BS];
    uint32_t id[BS];
    uint32_t hkey[HASH];
    uint16_t hslot[HASH];
    int n, E;
};
template <int BS> struct WideBwdSharedT {
    static constexpr int T = BS, WAVES = BS / 64, CAP = BS < WBK_CAP ? BS : WBK_CAP, LEVEL = BS > 128 ? 512 : 128;
    WBColT<BS> col[2];
    double fm[BS], fi[BS], fd[BS];  // the forward record
    uint32_t fid[BS];
    double dA[LEVEL], dB[LEVEL];  // level buffers; outside the column step: val = dA, order = dB, the list entries being
                                  // sorted = (dB, list)
    uint32_t list[LEVEL];
    double red[2][8];
    int wsum[2][8];
    double bterm[BS];  // per slot: its term of bib's sum over the list, init_v (p_IM e_v(x) m'[v] + p_ID d[v])
    double ib[2];      // InsBegin of B.tables[p], in its column's scale, by the parity of p
    unsigned long long bc;
    LinParams lp;  // (read from here: the scalar registers are short)
};
// (the names the one-size block had)
using WBCol = WBColT<WBK_T>;
using WideBwdShared = WideBwdSharedT<WBK_T>;

template <class Col> __device__ __forceinline__ uint32_t wb_hash(uint32_t id) { return (id * 2654435761u) >> Col::HASH_SHIFT; }
template <class Col> __device__ __forceinline__ void wb_insert(Col &c, uint32_t id, int slot) {
    uint32_t h = wb_hash<Col>(id);
    for (;;) {
        const uint32_t old = atomicCAS(&c.hkey[h], H_EMPTY, id);
        if (old == H_EMPTY) {
            c.hslot[h] = (uint16_t)slot;
            return;
        }
        if (old == id) return;
        h = (h + 1) & (Col::HASH - 1);
    }
}
template <class Col> __device__ __forceinline__ int wb_find(const Col &c, uint32_t id) {
    uint32_t h = wb_hash<Col>(id);
    for (;;) {
        const uint32_t k = c.hkey[h];
        if (k == id) return (int)c.hslot[h];
        if (k == H_EMPTY) return -1;
        h = (h + 1) & (Col::HASH - 1);
    }
}
// (`par` alternates between two sets of wave results: one barrier per reduction)
template <class Sh> __device__ __forceinline__ double wb_block_max(Sh &sh, int &par, double v) {  // non-negative values
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) sh.red[par][threadIdx.x >> 6] = v;
    __syncthreads();
    double r = sh.red[par][0];
#pragma unroll
    for (int w = 1; w < Sh::WAVES; w++) r = fmax(r, sh.red[par][w]);
    par ^= 1;
    return r;
}
template <class Sh> __device__ __forceinline__ int wb_block_isum(Sh &sh, int &par, int v) {
    v = wave_isum(v);
    if ((threadIdx.x & 63) == 0) sh.wsum[par][threadIdx.x >> 6] = v;
    __syncthreads();
    int r = 0;
#pragma unroll
    for (int w = 0; w < Sh::WAVES; w++) r += sh.wsum[par][w];
    par ^= 1;
    return r;
}

// forward record of a position into sh.f*; false: missing (or larger than the class)
template <class Sh>
__device__ __forceinline__ bool wb_load_record(const RecPool &p, uint64_t pos_index, Sh &sh, int &n, int &na, int &E) {
    const uint64_t o1 = p.off[pos_index];
    if (o1 == 0) return false;
    const uint8_t *rec = p.base + (o1 - 8);
    const int *hw = (const int *)rec;
    n = hw[0];
    na = hw[1];
    E = hw[2];
    if (n > Sh::CAP) return false;
    const uint64_t idb = (uint64_t)((n + 1) & ~1) * 4;
    const uint32_t *ids = (const uint32_t *)(rec + 16);
    const double *m = (const double *)(rec + 16 + idb), *i = m + na, *d = i + na;
    const int t = threadIdx.x;
    if (t < n) {
        sh.fid[t] = ids[t];
        sh.fd[t] = d[t];
        sh.fm[t] = t < na ? m[t] : 0.0;
        sh.fi[t] = t < na ? i[t] : 0.0;
    }
    __syncthreads();
    return true;
}

template <class Sh> __device__ __forceinline__ int wb_excl_scan(Sh &sh, int &par, int v, int &total) {
    const int inc = wave_iscan(v);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 63) sh.wsum[par][w] = inc;
    __syncthreads();
    int pre = 0, tt = 0;
#pragma unroll
    for (int k = 0; k < Sh::WAVES; k++) {
        const int x = sh.wsum[par][k];
        tt += x;
        pre += k < w ? x : 0;
    }
    total = tt;
    par ^= 1;
    return pre + inc - v;
}

// emit_mapping (mapping_flow.hip) with by_node = true, topk = 0: val[0..n) -> the list record of a position.  Only the
// entries that stay are sorted (a column next to a wide spot has 400 entries of which a few dozen stay).
template <class Sh>
__device__ __forceinline__ bool wb_emit(const RecPool &mp, uint64_t pos_index, Sh &sh, int &par, int n, double ratio_lin) {
    const int t = threadIdx.x;
    const double v = t < n ? sh.dA[t] : 0.0;
    double *val = sh.dB;       // the list being built: log values ...
    uint32_t *ids = sh.list;   // ... and node ids
    const double thr = wb_block_max(sh, par, v) * ratio_lin;
    const bool stay = t < n && v > 0.0 && v > thr;
    int keep;
    const int at = wb_excl_scan(sh, par, stay ? 1 : 0, keep);
    // the list is ordered by the values it holds -- the LOGS -- and equal logs by node id (emit_mapping)
    const int NP = bitonic_size(keep);
    if (stay) {
        val[at] = log(v);
        ids[at] = sh.fid[t];
    }
    for (int k = t; k < NP; k += Sh::T)
        if (k >= keep) {
            val[k] = -INFINITY;
            ids[k] = 0xffffffffu;
        }
    block_bitonic_desc(val, ids, NP);
    const uint64_t idb = (uint64_t)((keep + 1) & ~1) * 4;
    const uint64_t bytes = 8 + idb + (uint64_t)keep * 8;
    if (t == 0) sh.bc = atomicAdd(mp.top, (unsigned long long)bytes);
    __syncthreads();
    const uint64_t o = sh.bc;
    if (o + bytes > mp.cap) return false;
    uint8_t *rec = mp.base + o;
    if (t == 0) {
        ((uint32_t *)rec)[0] = (uint32_t)keep;
        ((uint32_t *)rec)[1] = 0;
        mp.off[pos_index] = o + 8;
    }
    uint32_t *oid = (uint32_t *)(rec + 8);
    double *olp = (double *)(rec + 8 + idb);
    if (t < keep) {
        oid[t] = ids[t];
        olp[t] = val[t];
    }
    __syncthreads();
    return true;
}

// The list flavour's arguments: a.cells is the call statistics' counter, list entries of the columns computed.
struct WideBwdListArgs : SparseBwdArgs {
    unsigned long long *cells;
};
// ... and those of its transition-posterior form
struct WideBwdEdgeArgs : SparseBwdEdgeArgs {
    unsigned long long *cells;
};
// ... and those of its state-posterior form
struct WideBwdStatesArgs : SparseBwdStatesArgs {
    unsigned long long *cells;
};
template <bool LIST, bool EDGES, bool STATES = false>
using WideBwdArgsOf = typename std::conditional<
    LIST,
    typename std::conditional<STATES, WideBwdStatesArgs, typename std::conditional<EDGES, WideBwdEdgeArgs, WideBwdListArgs>::type>::type,
    SparseBwdArgs>::type;

// (STATES) to_emit_probs of one merged index by state over the entries of the input list of read position rq
// (emit_states, mapping_flow.hip, thread = slot): sh.f* = F.tables[p] (fn entries, exponent fE), b = B.tables[p+1] with
// exponent Eb (null: b_init, p_end in every state of every node, exponent 0).  A thread keeps its list entry in a
// register and looks its node up in the record -- its own slot first, then the whole record -- and in b's hash.  The
// head of to_states() is a wave reduction over (value, kind, slot) and, across the waves, thread 0's pass over one
// pair per wave.  False: the list is longer than the block (the same for every thread).  Ends behind a barrier: the
// next step loads another record into sh.f*.
template <class Sh, class Col>
__device__ __forceinline__ bool wb_states(const SparseBwdStatesArgs &a, uint64_t rq, Sh &sh, int &par, int fn, int fE, const Col *b,
                                          int Eb, double logP, bool ok) {
    const int t = threadIdx.x;
    const uint64_t l0 = a.list_off[rq];
    const int nl = (int)(a.list_off[rq + 1] - l0);
    if (nl > Sh::CAP) return false;
    double bv = -INFINITY;
    int br = -1;
    if (t < nl) {
        const uint32_t v = a.list_nodes[l0 + t];
        const double pend = sh.lp.p_end;
        const double w = (double)(fE + Eb) * SP_LN2 - logP;
        int j = t < fn && sh.fid[t] == v ? t : -1;
        for (int q = 0; j < 0 && q < fn; q++)
            if (sh.fid[q] == v) j = q;
        double lm = -INFINITY, li = -INFINITY, ld = -INFINITY;
        if (ok && j >= 0) {
            double bm = pend, bi = pend, bd = pend;
            if (b) {
                const int bs = wb_find(*b, v);
                bm = bs >= 0 ? b->m[bs] : 0.0;
                bi = bs >= 0 ? b->i[bs] : 0.0;
                bd = bs >= 0 ? b->d[bs] : 0.0;
            }
            lm = st_log(sh.fm[j], bm, w);
            li = st_log(sh.fi[j], bi, w);
            ld = st_log(sh.fd[j], bd, w);
        }
        if (a.st_logp) {
            double *o = a.st_logp + 3 * (l0 + (uint64_t)t);
            o[0] = lm;
            o[1] = li;
            o[2] = ld;
        }
        st_take(bv, br, lm, t);
        st_take(bv, br, li, ST_RANK + t);
        st_take(bv, br, ld, 2 * ST_RANK + t);
    }
    st_wave_best(bv, br);
    if ((t & 63) == 0) {
        sh.red[par][t >> 6] = bv;
        sh.wsum[par][t >> 6] = br;
    }
    __syncthreads();
    if (t == 0 && a.st_best) {
#pragma unroll
        for (int w = 1; w < Sh::WAVES; w++) st_take(bv, br, sh.red[par][w], sh.wsum[par][w]);
        a.st_best[rq] = st_code(br);
    }
    par ^= 1;
    return true;
}

// (EDGES) The edge terms of merged index i for the forward entry in slot j of sh.f* (emit_edge_terms, mapping_flow.hip,
// thread = slot), one per child of the node in the CSR's order:
//   to Match (i < len): t e_l(x[i]) B.table_merged(i+1).m[l] (p_MM F.m[k] + p_IM F.i[k] + p_DM F.d[k]) / P   (weight wM)
//   to Del:             t           B.table_merged(i).d[l]   (p_MD F.m[k] + p_ID F.i[k] + p_DD F.d[k]) / P   (weight wD)
// prev_init: B.table_merged(i+1) is b_init, m = p_end on every node; i_is_len: the Del target is b_init (d = p_end), no
// Match term.  Returns the number of non-zero terms; STORE: writes them into the record from slot w on, keys = edge ids.
// The block counts first and stores after the scan of the counts: the terms are computed twice instead of held in
// registers across the scan (the kernel sits at its 128 VGPRs).
template <bool STORE, class Sh, class Col>
__device__ __forceinline__ int wb_edge_terms(const SparseBwdEdgeArgs &a, const Sh &sh, int j, const Col &prev, bool prev_init,
                                             const Col &cur, bool i_is_len, uint8_t x, double wM, double wD, uint64_t w) {
    const SparseModel &M = a.M;
    const LinParams &lp = sh.lp;
    const uint32_t k = sh.fid[j];
    const double fm = sh.fm[j], fi = sh.fi[j], fd = sh.fd[j];
    const double sm = lp.p_MM * fm + lp.p_IM * fi + lp.p_DM * fd;
    const double sd = lp.p_MD * fm + lp.p_ID * fi + lp.p_DD * fd;
    const uint32_t a0 = M.chi_off[k], deg = M.chi_off[k + 1] - a0;
    int c = 0;
#pragma unroll 1
    for (uint32_t q = 0; q < deg; q++) {
        const double tw = M.chi_w[a0 + q];
        const uint32_t l = M.chi_node[a0 + q];
        double term = 0.0;
        if (!i_is_len) {
            double bm = lp.p_end;
            if (!prev_init) {
                const int ps = wb_find(prev, l);
                bm = ps >= 0 ? prev.m[ps] : 0.0;
            }
            // (a zero factor stays zero whatever the weight: no 0 * inf)
            const double v1 = sm * (M.emis[l] == x ? lp.p_match : lp.p_mismatch) * bm;
            if (v1 != 0.0) term += v1 * wM;
        }
        double bd = lp.p_end;
        if (!i_is_len) {
            const int cs = wb_find(cur, l);
            bd = cs >= 0 ? cur.d[cs] : 0.0;
        }
        const double v2 = sd * bd;
        if (v2 != 0.0) term += v2 * wD;
        const double val = tw * term;
        if (val != 0.0) {
            if (STORE) {
                a.rec_key[w + c] = M.chi_edge[a0 + q];
                a.rec_val[w + c] = val;
            }
            c++;
        }
    }
    return c;
}

// (LIST: 4 waves per SIMD -- 128 VGPRs -- let two blocks of 448 share a CU, as the adaptive flavour's 127 do unasked)
template <bool LIST = false, bool EDGES = false, int BS = WBK_T, bool STATES = false>
__global__ void __launch_bounds__(BS, LIST ? 4 : 1) wide_backward_kernel(const WideBwdArgsOf<LIST, EDGES, STATES> a) {
    static_assert(LIST || (!EDGES && !STATES && BS == WBK_T), "the adaptive flavour has one size, no edge terms and no state posteriors");
    static_assert(!(EDGES && STATES), "one flavour at a time");
    static_assert(BS == WBK_T || BS == WBK_T_SMALL, "two block sizes");
    using Sh = WideBwdSharedT<BS>;
    using Col = WBColT<BS>;
    __shared__ Sh sh;
    const int t = threadIdx.x;
    const uint32_t gi = a.lanes[blockIdx.x];
    const int g = (int)(gi / a.W), r = (int)(gi % a.W);
    const int len = a.d.len[gi];
    const int s0 = a.sw[gi];
    const uint64_t p0 = a.lane_pos0[gi];
    const uint64_t q0 = a.map_pos0[gi];
    const double logP = a.d.logPf[gi];
    if (t == 0) sh.lp = a.M.lp;
    __syncthreads();
    const LinParams &lp = sh.lp;
    uint32_t err = 0;
    int par = 0;
    const bool ok = logP > -INFINITY;
    int pos;            // next position to compute
    int have_cols = 0;  // col[(pos+1)&1] holds B.tables[pos+1] (and sh.ib[(pos+1)&1] its InsBegin)
    bool stopped = false;
    int stop_at = 0;
    int fn = 0, fna = 0, fE = 0;
    // (LIST) MatchBegin and exponent of column 0 once it is computed, entries of the columns computed so far
    double mb0 = 0.0;
    int E0 = 0;
    bool done0 = false;
    unsigned long long n_cells = 0;
    uint64_t end_fill = 0;  // (EDGES) entries of merged index len, at the head of the record of position len-1
    if (LIST || a.mode == 0) {
        pos = len - 1;
        // merged index len: F.tables[len-1] (.) b_init / P   (table.rs:414-434, backward.rs:197-211)
        if (!wb_load_record(a.fpool, p0 + (uint64_t)(len - 1), sh, fn, fna, fE)) {
            stopped = true;  // missing: nothing done
            stop_at = len;
        } else if constexpr (EDGES) {
            // merged index len (Del into b_init only) opens the record of position len-1 (freq.rs:276-298)
            const uint64_t rq = q0 + (uint64_t)(len - 1);
            const uint64_t base = a.rec_off[rq], cap = a.rec_off[rq + 1] - base;
            const double wD = ok ? exp((double)fE * SP_LN2 - logP) : 0.0;
            int cnt = 0;
            if (ok && t < fn) cnt = wb_edge_terms<false>(a, sh, t, sh.col[0], true, sh.col[0], true, 0, 0.0, wD, 0);
            int tot;
            const int at = wb_excl_scan(sh, par, cnt, tot);
            if ((uint64_t)tot > cap) err |= SP_ERR_CAPACITY;  // (cannot happen: the bound is exact; nothing is written past the record)
            else {
                if (cnt) wb_edge_terms<true>(a, sh, t, sh.col[0], true, sh.col[0], true, 0, 0.0, wD, base + (uint64_t)at);
                end_fill = (uint64_t)tot;
            }
        } else if constexpr (STATES) {
            if (!wb_states<Sh, Col>(a, q0 + (uint64_t)(len - 1), sh, par, fn, fE, nullptr, 0, logP, ok)) err |= SP_ERR_CAPACITY;
        } else {
            const double w = ok ? exp((double)fE * SP_LN2 - logP) * lp.p_end : 0.0;
            if (t < fn) sh.dA[t] = w * (sh.fm[t] + sh.fi[t] + sh.fd[t]);
            __syncthreads();
            if (!wb_emit(a.mpool, q0 + (uint64_t)(len - 1), sh, par, fn, a.ratio_lin)) err |= SP_ERR_POOL;
        }
    } else {
        pos = a.stop[gi];
        if (pos < len - 1) {
            // B.tables[pos+1] from the hand-off slot
            const BHandoff &h = a.hand[gi];
            Col &c = sh.col[(pos + 1) & 1];
            const int n = h.n;
            for (int k = t; k < Col::HASH; k += BS) c.hkey[k] = H_EMPTY;
            if (t == 0) {
                c.n = n;
                c.E = h.E;
                sh.ib[(pos + 1) & 1] = h.ib;
            }
            __syncthreads();
            if (t < n) {
                c.id[t] = h.id[t];
                c.m[t] = h.m[t];
                c.i[t] = h.i[t];
                c.d[t] = h.d[t];
                wb_insert(c, h.id[t], t);
            }
            __syncthreads();
            have_cols = 1;
        }
    }
    int steps_done = 0;
    // (LIST) the walk goes on to position 0: B.tables[0] over mapping.nodes(0), begin states only
    for (; !stopped && pos >= (LIST ? 0 : s0 + 1) && !err; pos--) {
        // B.tables[pos] over filled_nodes(F.tables[pos-1]) (backward.rs:122-129)
        if ((!LIST || pos > 0) && !wb_load_record(a.fpool, p0 + (uint64_t)(pos - 1), sh, fn, fna, fE)) {
            stopped = true;
            stop_at = pos;
            break;
        }
        double *val = sh.dA;
        int nl;
        if constexpr (LIST) {
            // mapping.nodes(pos) (backward.rs:59-90)
            const uint64_t l0 = a.list_off[q0 + (uint64_t)pos];
            nl = (int)(a.list_off[q0 + (uint64_t)pos + 1] - l0);
            if (nl > Sh::CAP) {  // (the same for every thread)
                err |= SP_ERR_CAPACITY;
                break;
            }
            if (t < nl) sh.list[t] = a.list_nodes[l0 + t];
        } else {
            uint16_t *order = (uint16_t *)sh.dB;
            // filled_nodes (table.rs:117-123): the record's elements by total, stable (sort_desc, frontier_dev.h)
            {
                const int NP = bitonic_size(fn);
                for (int k = t; k < NP; k += BS) {
                    val[k] = k < fn ? sh.fm[k] + sh.fi[k] + sh.fd[k] : -1.0;
                    order[k] = (uint16_t)k;
                }
                block_bitonic_desc(val, order, NP);
            }
            nl = fna < fn ? fna : fn;
            if (t < nl) sh.list[t] = sh.fid[order[t]];
        }
        __syncthreads();
        // ---- one backward column over the list (bwd_list_step, sparse_dev.h)
        const Col &prev = sh.col[(pos + 1) & 1];
        Col &cur = sh.col[pos & 1];
        const bool prev_is_init = pos == len - 1;
        const uint8_t x = a.bases[((size_t)g * a.Lb + pos) * a.W + r];
        for (int k = t; k < Col::HASH; k += BS) cur.hkey[k] = H_EMPTY;
        if (t == 0) cur.n = nl;
        __syncthreads();
        BwdAdj rec;
        rec.nchi = 0;
        if (t < nl) {
            const uint32_t k = sh.list[t];
            cur.id[t] = k;
            wb_insert(cur, k, t);
            rec = a.M.badj[k];
        }
        __syncthreads();
        const double pend = lp.p_end;
        // bd0 (backward.rs:354-377); keep A1 = sum_w t e_w m'[w] and q0 = p_r i'[v] for bm/bi
        int cs[ADJ_DEG];
        double a1 = 0.0, qq = 0.0;
        if (t < nl) {
#pragma unroll
            for (int q = 0; q < ADJ_DEG; q++) {
                cs[q] = -1;
                if (q >= (int)rec.nchi) continue;
                const double w = rec.chi_w[q];
                if (w == 0.0) continue;
                const uint32_t u = rec.chi[q];
                double mu = 0.0;
                if (prev_is_init) mu = pend;
                else {
                    const int ps = wb_find(prev, u);
                    if (ps >= 0) mu = prev.m[ps];
                }
                a1 += w * (rec.chi_emis[q] == x ? lp.p_match : lp.p_mismatch) * mu;
                cs[q] = wb_find(cur, u);
            }
            double iv = 0.0, mv = 0.0;
            if (prev_is_init) iv = mv = pend;
            else {
                const int os = wb_find(prev, cur.id[t]);
                if (os >= 0) {
                    iv = prev.i[os];
                    mv = prev.m[os];
                }
            }
            qq = lp.p_random * iv;
            // bib (backward.rs:535-555), the m' half of this node's term: the node's own m'[v] sits in the slot the Ins term
            // just found; the d half is added at the rescale
            sh.bterm[t] = lp.p_IM * rec.init * (rec.emis == x ? lp.p_match : lp.p_mismatch) * mv;
            // (LIST) bmb (backward.rs:499-519) is wanted of column 0 alone: the same sum with p_MM / p_MD, in sh.fm --
            // position 0 has no forward record
            if (LIST && pos == 0) sh.fm[t] = lp.p_MM * rec.init * (rec.emis == x ? lp.p_match : lp.p_mismatch) * mv;
            const double d0 = lp.p_DM * a1 + lp.p_DI * qq;
            cur.d[t] = d0;
            sh.dA[t] = d0;
        }
        __syncthreads();
        // bdt (backward.rs:387-404), restricted to the list
        double *src = sh.dA, *dst = sh.dB;
        for (int lv = 1; lv <= lp.n_max_gaps; lv++) {
            if (t < nl) {
                double s = 0.0;
#pragma unroll
                for (int q = 0; q < ADJ_DEG; q++)
                    if (cs[q] >= 0) s += rec.chi_w[q] * src[cs[q]];
                s *= lp.p_DD;
                dst[t] = s;
                cur.d[t] += s;
            }
            __syncthreads();
            double *tmp = src;
            src = dst;
            dst = tmp;
        }
        // bm, bi: sum_w t (p_XM e_w m'[w] + p_XD d[w]) + p_XI p_r i'[v]
        double nm = 0.0, ni = 0.0, nd = 0.0;
        if (t < nl) {
            double td = 0.0;
#pragma unroll
            for (int q = 0; q < ADJ_DEG; q++)
                if (cs[q] >= 0) td += rec.chi_w[q] * cur.d[cs[q]];
            nm = lp.p_MM * a1 + lp.p_MD * td + lp.p_MI * qq;
            ni = lp.p_IM * a1 + lp.p_ID * td + lp.p_II * qq;
            nd = cur.d[t];
        }
        // rescale (col_rescale): the column maximum into [0.5, 1)
        const double mx = wb_block_max(sh, par, fmax(fmax(nm, ni), nd));
        const int e = sp_exp_of(mx);
        const double sc = sp_pow2(-e);
        const int Ecur = (prev_is_init ? 0 : prev.E) + e;
        if (t < nl) {
            cur.m[t] = nm * sc;
            cur.i[t] = ni * sc;
            cur.d[t] = nd * sc;
            sh.bterm[t] = (sh.bterm[t] + lp.p_ID * rec.init * nd) * sc;
            if (LIST && pos == 0) sh.fm[t] = (sh.fm[t] + lp.p_MD * rec.init * nd) * sc;
        }
        if (t == 0) cur.E = Ecur;
        __syncthreads();
        have_cols = 1;
        // bib = sum over the list of the terms + p_II p_r ib', in the column's scale, by wave 0 alone (its lane j adds the
        // slots j, j+64, ...): no block reduction, no barrier of its own
        if (t < 64) {  // (wave 0: the next barrier publishes sh.ib[pos & 1])
            double part = 0.0;
#pragma unroll 1
            for (int w = 0; w < Sh::WAVES; w++) {
                const int k = t + 64 * w;
                if (k < nl) part += sh.bterm[k];
            }
            const double ib = wave_sum(part) + lp.p_II * lp.p_random * (prev_is_init ? 0.0 : sh.ib[(pos + 1) & 1]) * sc;
            if (t == 0) sh.ib[pos & 1] = ib;
            if (LIST && pos == 0) {
                double pm = 0.0;
#pragma unroll 1
                for (int w = 0; w < Sh::WAVES; w++) {
                    const int k = t + 64 * w;
                    if (k < nl) pm += sh.fm[k];
                }
                mb0 = wave_sum(pm) + lp.p_MI * lp.p_random * (prev_is_init ? 0.0 : sh.ib[(pos + 1) & 1]) * sc;
            }
        }
        if constexpr (LIST) {
            n_cells += (unsigned long long)nl;
            if constexpr (EDGES) {
                // merged index pos: sh.f* = F.tables[pos-1], cur = B.tables[pos], prev = B.tables[pos+1] (b_init at len-1).
                // Edge terms by forward entry (none at pos 0), then the Begin terms (emit_begin_terms, mapping_flow.hip) by
                // slot of cur, then of prev unless it is b_init (dense there: the host adds it):
                //   to Del:   c_D init_v B.tables[pos].d[v] / P;   to Match: c_M init_v e_v(x[pos]) B.tables[pos+1].m[v] / P
                // with (c_M, c_D) = (p_MM, p_MD) at pos 0 and ib_{pos-1} (p_IM, p_ID) after, the chain in the exponent.
                const uint64_t rq = q0 + (uint64_t)pos;
                const uint64_t base = a.rec_off[rq], cap = a.rec_off[rq + 1] - base;
                const uint64_t fill = prev_is_init ? end_fill : 0;
                double bcur = 0.0, bprev = 0.0, wM = 0.0, wD = 0.0;
                int cnt = 0;
                if (ok) {
                    const int Eprev = prev_is_init ? 0 : prev.E;
                    if (pos > 0) {
                        wM = exp((double)(fE + Eprev) * SP_LN2 - logP);
                        wD = exp((double)(fE + Ecur) * SP_LN2 - logP);
                        if (t < fn) cnt = wb_edge_terms<false>(a, sh, t, prev, prev_is_init, cur, false, x, wM, wD, 0);
                    }
                    const double lib = pos == 0 ? 0.0 : a.M.logib[pos - 1];
                    const double cM = pos == 0 ? lp.p_MM : lp.p_IM, cD = pos == 0 ? lp.p_MD : lp.p_ID;
                    if (t < nl) {
                        const double v2 = a.M.init[cur.id[t]] * cD * cur.d[t];
                        if (v2 != 0.0) bcur = v2 * exp(lib + (double)Ecur * SP_LN2 - logP);
                    }
                    if (!prev_is_init && t < prev.n) {
                        const uint32_t v = prev.id[t];
                        const double v1 = a.M.init[v] * cM * (a.M.emis[v] == x ? lp.p_match : lp.p_mismatch) * prev.m[t];
                        if (v1 != 0.0) bprev = v1 * exp(lib + (double)Eprev * SP_LN2 - logP);
                    }
                }
                // one scan for the three groups: edge terms in bits 0-11 (at most ADJ_DEG x 448 = 2240), cur's and prev's Begin
                // terms in bits 12-21 and 22-31 (at most 448 each)
                int tot;
                const int at = wb_excl_scan(sh, par, cnt | (bcur != 0.0 ? 1 << 12 : 0) | (bprev != 0.0 ? 1 << 22 : 0), tot);
                const uint64_t nE = (uint64_t)(tot & 0xfff), nC = (uint64_t)((tot >> 12) & 0x3ff), nP = (uint64_t)((tot >> 22) & 0x3ff);
                if (fill + nE + nC + nP > cap) err |= SP_ERR_CAPACITY;  // (cannot happen: the bound is exact)
                else {
                    if (cnt) wb_edge_terms<true>(a, sh, t, prev, prev_is_init, cur, false, x, wM, wD, base + fill + (uint64_t)(at & 0xfff));
                    if (bcur != 0.0) {
                        const uint64_t w = base + fill + nE + (uint64_t)((at >> 12) & 0x3ff);
                        a.rec_key[w] = a.E + cur.id[t];
                        a.rec_val[w] = bcur;
                    }
                    if (bprev != 0.0) {
                        const uint64_t w = base + fill + nE + nC + (uint64_t)((at >> 22) & 0x3ff);
                        a.rec_key[w] = a.E + prev.id[t];
                        a.rec_val[w] = bprev;
                    }
                    if (t == 0) a.rec_cnt[rq] = fill + nE + nC + nP;
                }
            }
            if (pos == 0) {  // column 0 has no F.tables[-1]: nothing to emit
                E0 = Ecur;
                done0 = true;
                break;
            }
            if constexpr (EDGES) continue;  // no mapping list
            if constexpr (STATES) {
                // merged index pos >= 1 belongs to read position pos-1: sh.f* = F.tables[pos-1], cur = B.tables[pos]
                if (!wb_states<Sh, Col>(a, q0 + (uint64_t)(pos - 1), sh, par, fn, fE, &cur, Ecur, logP, ok)) err |= SP_ERR_CAPACITY;
                continue;  // no mapping list
            }
        }
        // S = F.tables[pos-1] (.) B.tables[pos] / P over F's elements (table.rs:320-345, 500-505)
        const double w = ok ? exp((double)(fE + Ecur) * SP_LN2 - logP) : 0.0;
        if (t < fn) {
            const int bs = wb_find(cur, sh.fid[t]);
            val[t] = bs >= 0 ? w * (sh.fm[t] * cur.m[bs] + sh.fi[t] * cur.i[bs] + sh.fd[t] * cur.d[bs]) : 0.0;
        }
        __syncthreads();
        if (!wb_emit(a.mpool, q0 + (uint64_t)(pos - 1), sh, par, fn, a.ratio_lin)) err |= SP_ERR_POOL;
        // a burst (max_steps) ends where the column fits the one-lane-per-node class again
        if (!LIST && a.max_steps > 0 && !err && ++steps_done >= a.max_steps && nl <= 64 && pos - 1 >= s0 + 1) {
            stopped = true;
            stop_at = pos - 1;
            break;
        }
    }
    if constexpr (LIST) {
        if (stopped) err |= SP_ERR_CAPACITY;  // a forward record is missing or larger than the block
        if (t == 0) {
            a.stop[gi] = stopped ? stop_at : s0;
            // ln B.tables[0].mb
            if (a.logb && done0 && !err) a.logb[gi] = log(mb0) + (double)E0 * SP_LN2;
            if (a.cells && n_cells) atomicAdd(a.cells, n_cells);
        }
    } else if (stopped && !err) {
        // park B.tables[stop_at + 1] for the next phase
        if (have_cols && stop_at < len) {
            const Col &c = sh.col[(stop_at + 1) & 1];
            BHandoff &h = a.hand[gi];
            if (c.n > HANDOFF_CAP) err |= SP_ERR_CAPACITY;
            else {
                if (t == 0) {
                    h.n = c.n;
                    h.E = c.E;
                    h.ib = sh.ib[(stop_at + 1) & 1];
                }
                if (t < c.n) {
                    h.id[t] = c.id[t];
                    h.m[t] = c.m[t];
                    h.i[t] = c.i[t];
                    h.d[t] = c.d[t];
                }
            }
        }
        if (t == 0) a.stop[gi] = stop_at;
    } else if (!err) {
        // hand B.tables[s0+1] to the dense backward kernel: dense column (zeros elsewhere), its exponent and maximum
        if (have_cols) {
            const Col &c = sh.col[(s0 + 1) & 1];
            const size_t NW = (size_t)a.d.N * a.W;
            const int pc = (s0 + 1) & 1;
            double *bm = a.d.Bm + ((size_t)g * a.d.bcols + pc) * NW;
            double *bi = a.d.Bi + ((size_t)g * a.d.bcols + pc) * NW;
            double mx = 0.0;
            if (t < c.n) {
                bm[(size_t)c.id[t] * a.W + r] = c.m[t];
                bi[(size_t)c.id[t] * a.W + r] = c.i[t];
                if (a.d.skH && (c.m[t] != 0.0 || c.i[t] != 0.0))  // (run skipping, dense.hip: the segment counts from column s0 on)
                    atomicOr(&a.d.skH[(size_t)g * a.d.nseg + c.id[t] / (uint32_t)a.d.sseg], 1u << (s0 + 1 < 31 ? s0 + 1 : 31));
                mx = fmax(c.m[t], c.i[t]);
            }
            mx = wb_block_max(sh, par, mx);
            if (t == 0) {
                a.d.cmaxB[((size_t)g * a.d.Lc + (s0 + 1)) * a.W + r] = (unsigned long long)__double_as_longlong(mx);
                a.d.BE[((size_t)g * (a.d.Lc + 1) + (s0 + 1)) * a.W + r] = c.E;
                // its InsBegin, natural log, for the dense head's begin-state chain (bwd_chain, dense.hip)
                a.d.logibB[((size_t)g * (a.d.Lc + 1) + (s0 + 1)) * a.W + r] = log(sh.ib[(s0 + 1) & 1]) + (double)c.E * SP_LN2;
            }
        }
        if (t == 0) a.stop[gi] = s0;
    }
    if (t == 0) a.err[gi] = err;
}


}  // namespace phmm
