// The weighted walk over mapping lists (phmm_run_with_mapping_weighted_path, include/phmm_amd_mea.h) and the kernels
// of the maximum-expected-accuracy call in front of it.
//
// mea_forward_kernel<CAP, HASH>: best_path_forward_kernel (best_path_kernel.h) with the roles of the numbers changed.
// The model's logs only say which transitions exist (a term > -inf: admissible); the value of a state is its own
// weight, read per entry from global memory, plus the largest value among its admissible sources -- one double addition
// per state, fl(source + own weight), so a path's value is its weights summed left to right.  Same layout: one wave64 per
// read, the previous and the current column in LDS with a hash node -> first slot each, the <= 64 class at one lane per
// entry and the 400 class looping the column, G + 1 Del levels in two LDS rows that swap.  Same ranks and the same
// 16-byte BpRec records, so best_path_traceback_kernel walks them back unchanged.  -inf means "no admissible path
// reaches the state" and nothing else: the weights are finite (mea_check_weights runs first), and no index is ever
// derived from a weight.
//
// mea_check_weights: flags any weight that is NaN or infinite.  mea_weights_from_states: the posteriors of the states
// pass, in place, to weights: exp of Match and Ins, del_weight * exp of Del, exp(-inf) = 0 exactly.
#pragma once

#include "best_path_kernel.h"

namespace phmm {

struct MeaArgs {
    BestPathArgs b;          // logp: the score
    const double *weights;   // [total_entries][3] Match, Ins, Del
    const double *ib_weight; // [total_bases] or null (0)
};

// the source's value if the transition exists, -inf otherwise
__device__ __forceinline__ double mea_via(double term, double v) { return term > -INFINITY ? v : -INFINITY; }

template <int CAP, int HASH>
__global__ void __launch_bounds__(64) mea_forward_kernel(const MeaArgs ma) {
    typedef BpCol<CAP, HASH> BCol;
    static_assert(HASH >= 2 * CAP && (HASH & (HASH - 1)) == 0, "hash at half load at most");
    __shared__ BCol cols[2];
    __shared__ double lv[2][CAP];  // Del level t - 1 and t
    __shared__ uint32_t rx[CAP], ry[CAP], rz[CAP], rw[CAP];
    const BestPathArgs &a = ma.b;
    const int lane = threadIdx.x;
    const uint32_t rd = a.read_ids[blockIdx.x];
    const BpParams &lp = a.lp;
    const uint64_t b0 = a.read_off[rd], len = a.read_off[rd + 1] - b0;
    const bool emit_i = lp.p_random > -INFINITY;  // Ins and InsBegin emit at all
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
        // Match and Ins from the previous column (column -1: Begin = 0, InsBegin = -inf, no node values)
        const double beg_v = pos == 0 ? 0.0 : ib, beg_t = pos == 0 ? lp.p_MM : lp.p_IM;
        for (int j = lane; j < n; j += 64) {
            const uint32_t k = C.id[j];
            const double *w = ma.weights + 3 * (e0 + j);
            double bv = -INFINITY;
            uint32_t br = BP_NO_RANK;
            if (np > 0)
                for (uint32_t e = a.par_off[k]; e < a.par_off[k + 1]; e++) {
                    const int q = bp_find(P, a.par_node[e]);
                    if (q < 0) continue;
                    const double t = a.trans_log[a.par_edge[e]];
                    bp_take(bv, br, mea_via(t + lp.p_MM, P.m[q]), ((uint32_t)q << 2) | 0u);
                    bp_take(bv, br, mea_via(t + lp.p_IM, P.i[q]), ((uint32_t)q << 2) | 1u);
                    bp_take(bv, br, mea_via(t + lp.p_DM, P.d[q]), ((uint32_t)q << 2) | 2u);
                }
            bp_take(bv, br, mea_via(a.init_log[k] + beg_t, beg_v), BP_BEGIN_M);
            const double mv = mea_via(a.emis[k] == x ? lp.p_match : lp.p_mismatch, bv) + w[0];
            C.m[j] = mv;
            uint32_t w0 = mv > -INFINITY ? (br & 0x7ffu) | (1u << 11) : 0u;
            const int me = np > 0 ? bp_find(P, k) : -1;
            double iv = -INFINITY;
            uint32_t ir = BP_NO_RANK;
            if (me >= 0 && emit_i) {
                bp_take(iv, ir, mea_via(lp.p_MI, P.m[me]), 0u);
                bp_take(iv, ir, mea_via(lp.p_II, P.i[me]), 1u);
                bp_take(iv, ir, mea_via(lp.p_DI, P.d[me]), 2u);
            }
            iv = iv + w[1];
            C.i[j] = iv;
            if (iv > -INFINITY) w0 |= ((ir & 3u) << 12) | (1u << 14);
            rx[j] = w0;
            rw[j] = me >= 0 ? (uint32_t)me : 0u;
        }
        // InsBegin of this column: from Begin at base 0, from InsBegin of the previous column behind it
        ib = emit_i ? mea_via(pos == 0 ? lp.p_MI : lp.p_II, pos == 0 ? 0.0 : ib) + (ma.ib_weight ? ma.ib_weight[b0 + pos] : 0.0)
                    : -INFINITY;
        wave_sync();
        // Del level 0 from this column's Match and Ins, and from InsBegin of this column
        for (int j = lane; j < n; j += 64) {
            const uint32_t k = C.id[j];
            const double wd = ma.weights[3 * (e0 + j) + 2];
            double bv = -INFINITY;
            uint32_t br = BP_NO_RANK;
            for (uint32_t e = a.par_off[k]; e < a.par_off[k + 1]; e++) {
                const int q = bp_find(C, a.par_node[e]);
                if (q < 0) continue;
                const double t = a.trans_log[a.par_edge[e]];
                bp_take(bv, br, mea_via(t + lp.p_MD, C.m[q]), ((uint32_t)q << 1) | 0u);
                bp_take(bv, br, mea_via(t + lp.p_ID, C.i[q]), ((uint32_t)q << 1) | 1u);
            }
            bp_take(bv, br, mea_via(a.init_log[k] + lp.p_ID, ib), BP_BEGIN_D);
            bv = bv + wd;
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
                const double wd = ma.weights[3 * (e0 + j) + 2];
                double bv = -INFINITY;
                uint32_t br = BP_NO_RANK;
                for (uint32_t e = a.par_off[k]; e < a.par_off[k + 1]; e++) {
                    const int q = bp_find(C, a.par_node[e]);
                    if (q < 0) continue;
                    bp_take(bv, br, mea_via(a.trans_log[a.par_edge[e]] + lp.p_DD, src[q]), (uint32_t)q);
                }
                bv = bv + wd;
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
    // the score: the largest of the last column's 3n values, if the model lets a path end
    double bv = -INFINITY;
    uint32_t br = BP_NO_RANK;
    if (!bad && len > 0 && lp.p_end > -INFINITY) {
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
        a.logp[rd] = bad ? NAN : bv;
        a.end_state[rd] = bv > -INFINITY ? br : BP_NO_RANK;
        a.err[rd] = bad ? BP_ERR_CAPACITY : 0u;
    }
}

// *flag = 1 if any of the n doubles is NaN or infinite (flag cleared by the host)
__global__ void __launch_bounds__(256) mea_check_weights(const double *w, uint64_t n, uint32_t *flag) {
    bool bad = false;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const double v = w[i];
        bad = bad || !(v - v == 0.0);
    }
    if (bad) atomicOr(flag, 1u);
}

// w[a][s] = exp(ln posterior), the Del column times del_weight; exp(-inf) = 0 exactly, and 0 * del_weight = 0
__global__ void __launch_bounds__(256) mea_weights_from_states(double *w, uint64_t n, double del_weight) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const double l = w[i];
        const double p = l > -INFINITY ? exp(l) : 0.0;
        w[i] = i % 3 == 2 ? del_weight * p : p;
    }
}

}  // namespace phmm
