// The best path over mapping lists (phmm_run_with_mapping_best_path): forward_with_mapping (forward.rs:51-75, f_step
// 276-306) with every sum replaced by a maximum, in the log domain, and the walk back through what each maximum chose.
//
// best_path_forward_kernel<CAP, HASH>: one wave64 per read, laid out as hinted_exact_kernel (sparse.hip) -- the column of
// the previous and of the current position in LDS with a hash node -> slot each; the <= 64 class has one lane per list
// entry, the 400 class loops the column.  Adds and maxima only: no scaling, no exp / log, and -inf is an ordinary value
// (nothing is ever subtracted, so no NaN can form).  The G + 1 Del levels are kept apart in two LDS rows that swap; D of an
// entry is the maximum over its levels.  Every entry leaves one 16-byte record of back-pointers (BpRec below).
//
// best_path_traceback_kernel: one lane per read, from the best end state back to base 0 through those records; it
// writes every row of out_path once and the four counts of the read.
//
// THE TIE RULE (include/phmm_amd_path.h): a maximum is taken over candidates with a rank each; a candidate replaces
// the one held when its value is greater, or equal and its rank LOWER; -inf never wins.  Ranks: an emitting source or an end
// state (slot << 2) | kind with kind 0 Match, 1 Ins, 2 Del -- the earlier slot first, within a slot Match before Ins
// before Del --, Begin behind every node state; a Del level's parent by its slot; among the Del levels the lower one.
#pragma once

#include "sparse_dev.h"

namespace phmm {

struct BpParams {  // natural logs, as phmm_params holds them
    double p_mismatch, p_match, p_random, p_end;
    double p_MM, p_IM, p_DM, p_MI, p_II, p_DI, p_MD, p_ID, p_DD;
    int G;  // n_max_gaps
};

// Back-pointers of one list entry, 16 bytes:
//   x  [0..10]  source of Match: (slot << 2) | kind in the previous list, BP_BEGIN_M = Begin   [11] Match is finite
//      [12..13] source kind of Ins (the same node in the previous list, its slot in w)          [14] Ins is finite
//      [15..17] the Del level that holds the maximum                                            [18] Del is finite
//      [19..28] source of Del level 0: (slot << 1) | (0 Match, 1 Ins) in this list, BP_BEGIN_D = InsBegin of this column
//   y  parent slot of Del levels 1, 2, 3 (9 bits each, this list);  z  of levels 4, 5, 6
//   w  [0..8] slot of the node in the previous list (source of Ins)
// A field of a state whose value is -inf is never followed.
static constexpr uint32_t BP_BEGIN_M = 0x7ffu, BP_BEGIN_D = 0x3ffu;
static constexpr uint32_t BP_NO_RANK = 0xffffffffu;
static constexpr uint32_t BP_ERR_CAPACITY = 1u, BP_ERR_WALK = 2u;

struct BestPathArgs {
    // the model: parents by CSR with edge ids (degree <= 8), init / trans in natural logs as the model was given them
    const uint8_t *emis;
    const uint32_t *par_off, *par_node, *par_edge;
    const double *init_log, *trans_log;
    BpParams lp;
    const uint8_t *bases;
    const uint64_t *read_off;     // [R+1]
    const uint64_t *map_pos_off;  // [total_bases+1]
    const uint32_t *map_nodes;
    const uint32_t *read_ids;     // forward: the reads of this launch's capacity class
    uint64_t ent0;                // first list entry of the chunk: record of entry a is rec[a - ent0]
    uint4 *rec;
    double *logp;                 // [R]
    uint32_t *end_state;          // [R] (slot << 2) | kind of the best end state, PHMM_PATH_NONE
    uint32_t *err;                // [R]
    // traceback
    uint32_t r0, r1;              // reads of the chunk
    uint64_t row0;                // first base of the chunk: row of base g is path[(g - row0) * stride]
    uint32_t *path;               // or null
    uint32_t stride;
    uint32_t *counts;             // [R][4] or null
};

__device__ __forceinline__ void bp_take(double &bv, uint32_t &br, double v, uint32_t rank) {
    if (v > bv || (v == bv && rank < br && v > -INFINITY)) {
        bv = v;
        br = rank;
    }
}

template <int CAP, int HASH> struct BpCol {
    double m[CAP], i[CAP], d[CAP];
    uint32_t id[CAP];
    uint32_t hkey[HASH];
    uint32_t hval[HASH];  // the FIRST slot that lists the node (a node listed twice is looked up there)
};
template <int CAP, int HASH> __device__ __forceinline__ int bp_find(const BpCol<CAP, HASH> &c, uint32_t key) {
    uint32_t h = ((key * 2654435761u) >> 16) & (HASH - 1);
    for (;;) {
        const uint32_t k = c.hkey[h];
        if (k == key) return (int)c.hval[h];
        if (k == H_EMPTY) return -1;
        h = (h + 1) & (HASH - 1);
    }
}

template <int CAP, int HASH>
__global__ void __launch_bounds__(64) best_path_forward_kernel(const BestPathArgs a) {
    typedef BpCol<CAP, HASH> BCol;
    static_assert(HASH >= 2 * CAP && (HASH & (HASH - 1)) == 0, "hash at half load at most");
    __shared__ BCol cols[2];
    __shared__ double lv[2][CAP];  // Del level t - 1 and t
    __shared__ uint32_t rx[CAP], ry[CAP], rz[CAP], rw[CAP];
    const int lane = threadIdx.x;
    const uint32_t rd = a.read_ids[blockIdx.x];
    const BpParams &lp = a.lp;
    const uint64_t b0 = a.read_off[rd], len = a.read_off[rd + 1] - b0;
    double ib = -INFINITY;  // InsBegin of the previous column
    int np = 0, cur = 0;
    bool bad = false;
    for (uint64_t pos = 0; pos < len; pos++, cur ^= 1) {
        BCol &C = cols[cur];
        const BCol &P = cols[cur ^ 1];
        const uint64_t e0 = a.map_pos_off[b0 + pos];
        const int n = (int)(a.map_pos_off[b0 + pos + 1] - e0);
        if (n > CAP) {
            bad = true;
            break;
        }
        const uint8_t x = a.bases[b0 + pos];
        for (int h = lane; h < HASH; h += 64) {
            C.hkey[h] = H_EMPTY;
            C.hval[h] = 0xffffffffu;
        }
        wave_sync();
        for (int j = lane; j < n; j += 64) {
            const uint32_t k = a.map_nodes[e0 + j];
            C.id[j] = k;
            uint32_t h = ((k * 2654435761u) >> 16) & (HASH - 1);
            for (;;) {
                const uint32_t old = atomicCAS(&C.hkey[h], H_EMPTY, k);
                if (old == H_EMPTY || old == k) {
                    atomicMin(&C.hval[h], (uint32_t)j);
                    break;
                }
                h = (h + 1) & (HASH - 1);
            }
        }
        wave_sync();
        // Match and Ins from the previous column (column -1: MB = 0, IB = -inf, no node values)
        const double beg_m = pos == 0 ? lp.p_MM : lp.p_IM + ib;
        for (int j = lane; j < n; j += 64) {
            const uint32_t k = C.id[j];
            double bv = -INFINITY;
            uint32_t br = BP_NO_RANK;
            if (np > 0)
                for (uint32_t e = a.par_off[k]; e < a.par_off[k + 1]; e++) {
                    const int q = bp_find(P, a.par_node[e]);
                    if (q < 0) continue;
                    const double t = a.trans_log[a.par_edge[e]];
                    bp_take(bv, br, t + (lp.p_MM + P.m[q]), ((uint32_t)q << 2) | 0u);
                    bp_take(bv, br, t + (lp.p_IM + P.i[q]), ((uint32_t)q << 2) | 1u);
                    bp_take(bv, br, t + (lp.p_DM + P.d[q]), ((uint32_t)q << 2) | 2u);
                }
            bp_take(bv, br, a.init_log[k] + beg_m, BP_BEGIN_M);
            const double mv = (a.emis[k] == x ? lp.p_match : lp.p_mismatch) + bv;
            C.m[j] = mv;
            uint32_t w0 = mv > -INFINITY ? (br & 0x7ffu) | (1u << 11) : 0u;
            const int me = np > 0 ? bp_find(P, k) : -1;
            double iv = -INFINITY;
            uint32_t ir = BP_NO_RANK;
            if (me >= 0) {
                bp_take(iv, ir, lp.p_MI + P.m[me], 0u);
                bp_take(iv, ir, lp.p_II + P.i[me], 1u);
                bp_take(iv, ir, lp.p_DI + P.d[me], 2u);
            }
            iv = lp.p_random + iv;
            C.i[j] = iv;
            if (iv > -INFINITY) w0 |= ((ir & 3u) << 12) | (1u << 14);
            rx[j] = w0;
            rw[j] = me >= 0 ? (uint32_t)me : 0u;
        }
        // IB of this column (MB of it is -inf)
        ib = lp.p_random + (pos == 0 ? lp.p_MI : lp.p_II + ib);
        wave_sync();
        // Del level 0 from this column's Match and Ins, and from InsBegin of this column
        const double beg_d = lp.p_ID + ib;
        for (int j = lane; j < n; j += 64) {
            const uint32_t k = C.id[j];
            double bv = -INFINITY;
            uint32_t br = BP_NO_RANK;
            for (uint32_t e = a.par_off[k]; e < a.par_off[k + 1]; e++) {
                const int q = bp_find(C, a.par_node[e]);
                if (q < 0) continue;
                const double t = a.trans_log[a.par_edge[e]];
                bp_take(bv, br, t + (lp.p_MD + C.m[q]), ((uint32_t)q << 1) | 0u);
                bp_take(bv, br, t + (lp.p_ID + C.i[q]), ((uint32_t)q << 1) | 1u);
            }
            bp_take(bv, br, a.init_log[k] + beg_d, BP_BEGIN_D);
            lv[0][j] = bv;
            C.d[j] = bv;  // best level so far: 0
            rx[j] |= (br & 0x3ffu) << 19;
            ry[j] = 0u;
            rz[j] = 0u;
        }
        // Del levels 1 .. G: a path through level t comes from level t - 1
        for (int t = 1; t <= lp.G; t++) {
            wave_sync();
            const double *src = lv[(t - 1) & 1];
            double *dst = lv[t & 1];
            for (int j = lane; j < n; j += 64) {
                const uint32_t k = C.id[j];
                double bv = -INFINITY;
                uint32_t br = BP_NO_RANK;
                for (uint32_t e = a.par_off[k]; e < a.par_off[k + 1]; e++) {
                    const int q = bp_find(C, a.par_node[e]);
                    if (q < 0) continue;
                    bp_take(bv, br, a.trans_log[a.par_edge[e]] + (lp.p_DD + src[q]), (uint32_t)q);
                }
                dst[j] = bv;
                if (bv > -INFINITY) {
                    const uint32_t f = (br & 0x1ffu) << (9 * ((t - 1) % 3));
                    if (t <= 3) ry[j] |= f;
                    else rz[j] |= f;
                }
                if (bv > C.d[j]) {  // (equal: the lower level stands)
                    C.d[j] = bv;
                    rx[j] = (rx[j] & ~(7u << 15)) | ((uint32_t)t << 15);
                }
            }
        }
        // (rx / ry / rz / rw of entry j are written and read by the lane that owns j only)
        for (int j = lane; j < n; j += 64) {
            const uint32_t w0 = rx[j] | (C.d[j] > -INFINITY ? 1u << 18 : 0u);
            a.rec[e0 - a.ent0 + j] = make_uint4(w0, ry[j], rz[j], rw[j]);
        }
        wave_sync();
        np = n;
    }
    // best = p_end + the largest of the last column's 3n values
    double bv = -INFINITY;
    uint32_t br = BP_NO_RANK;
    if (!bad && len > 0) {
        const BCol &L = cols[cur ^ 1];
        for (int j = lane; j < np; j += 64) {
            bp_take(bv, br, L.m[j], ((uint32_t)j << 2) | 0u);
            bp_take(bv, br, L.i[j], ((uint32_t)j << 2) | 1u);
            bp_take(bv, br, L.d[j], ((uint32_t)j << 2) | 2u);
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double ov = __shfl_xor(bv, off);
            const uint32_t orr = (uint32_t)__shfl_xor((int)br, off);
            bp_take(bv, br, ov, orr);
        }
    }
    if (lane == 0) {
        a.logp[rd] = bad ? NAN : lp.p_end + bv;
        a.end_state[rd] = lp.p_end + bv > -INFINITY ? br : BP_NO_RANK;
        a.err[rd] = bad ? BP_ERR_CAPACITY : 0u;
    }
}

// One lane per read of the chunk.  A row is entry 0 = the emitting state, then the Del states behind it in the order
// the path passes them, then PHMM_PATH_NONE; it is put together in registers and stored once.  (static, as the offsets
// kernel below: mea_path.hip launches the two as well.)
static __global__ void __launch_bounds__(64) best_path_traceback_kernel(const BestPathArgs a) {
    const uint32_t rd = a.r0 + blockIdx.x * 64 + threadIdx.x;
    if (rd >= a.r1) return;
    const uint64_t b0 = a.read_off[rd], len = a.read_off[rd + 1] - b0;
    const uint32_t stride = a.stride;
    uint32_t cnt[4] = {0, 0, 0, 0};
    uint32_t state = a.end_state[rd];
    uint32_t err = 0;
    if (a.err[rd]) state = BP_NO_RANK;
    if (state == BP_NO_RANK) {
        if (a.path)
            for (uint64_t p = 0; p < len; p++)
                for (uint32_t c = 0; c < stride; c++) a.path[(b0 + p - a.row0) * stride + c] = 0xffffffffu;
    } else {
        // state: (slot << 2) | kind of a state of column p, or BP_BEGIN_M = InsBegin of column p
        for (uint64_t p = len; p-- > 0;) {
            const uint64_t e0 = a.map_pos_off[b0 + p];
            const uint32_t n = (uint32_t)(a.map_pos_off[b0 + p + 1] - e0);
            const uint4 *rec = a.rec + (e0 - a.ent0);
            uint32_t row[8];
#pragma unroll
            for (int c = 0; c < 8; c++) row[c] = 0xffffffffu;
            uint32_t n_del = 0;
            if (state != BP_BEGIN_M && (state & 3u) == 2u) {
                // the Del chain of this column: from the level that holds the maximum down to level 0
                uint32_t slot = state >> 2;
                if (slot >= n) {
                    err = BP_ERR_WALK;
                    break;
                }
                uint4 r = rec[slot];
                const uint32_t T = (r.x >> 15) & 7u;
                n_del = T + 1;
                if (n_del + 1 > stride) {
                    err = BP_ERR_WALK;
                    break;
                }
                for (uint32_t t = T;; t--) {
                    const uint32_t code = (slot << 2) | 2u;
#pragma unroll
                    for (int c = 1; c < 8; c++)
                        if ((uint32_t)c == t + 1) row[c] = code;
                    if (t == 0) break;
                    slot = ((t <= 3 ? r.y : r.z) >> (9 * ((t - 1) % 3))) & 0x1ffu;
                    if (slot >= n) {
                        err = BP_ERR_WALK;
                        break;
                    }
                    r = rec[slot];
                }
                if (err) break;
                const uint32_t s0 = (r.x >> 19) & 0x3ffu;
                state = s0 == BP_BEGIN_D ? BP_BEGIN_M : ((s0 >> 1) << 2) | (s0 & 1u);
            }
            // the emitting state of base p and the state it came from
            uint32_t prev;
            if (state == BP_BEGIN_M) {
                row[0] = 0xfffffffdu;  // PHMM_PATH_INS_BEGIN
                cnt[2]++;
                prev = BP_BEGIN_M;  // (InsBegin of column p - 1; at p = 0 it came from Begin)
            } else {
                const uint32_t slot = state >> 2;
                if (slot >= n) {
                    err = BP_ERR_WALK;
                    break;
                }
                const uint4 r = rec[slot];
                row[0] = state;
                if ((state & 3u) == 0u) {
                    cnt[a.emis[a.map_nodes[e0 + slot]] == a.bases[b0 + p] ? 0 : 1]++;
                    prev = r.x & 0x7ffu;  // BP_BEGIN_M: Begin at p = 0, InsBegin of column p - 1 otherwise
                } else {
                    cnt[2]++;
                    prev = ((r.w & 0x1ffu) << 2) | ((r.x >> 12) & 3u);
                }
            }
            cnt[3] += n_del;
            if (a.path) {
                uint32_t *out = a.path + (b0 + p - a.row0) * stride;
#pragma unroll
                for (int c = 0; c < 8; c++)
                    if ((uint32_t)c < stride) out[c] = row[c];
            }
            state = prev;
        }
    }
    if (err) a.err[rd] = err;
    if (a.counts)
        for (int c = 0; c < 4; c++) a.counts[(size_t)rd * 4 + c] = err ? 0u : cnt[c];
}

// first list entry of every read (and the total behind the last)
static __global__ void __launch_bounds__(256) best_path_entry_offsets(const uint64_t *read_off, const uint64_t *map_pos_off,
                                                               uint64_t R, uint64_t *out) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r <= R) out[r] = map_pos_off[read_off[r]];
}

}  // namespace phmm
