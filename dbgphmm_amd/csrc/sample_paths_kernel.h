// Posterior path samples over mapping lists (phmm_run_with_mapping_sample_paths): the recursion of best_path_kernel.h
// with every maximum replaced by a log-sum-exp, and one random walk back per sample.  include/phmm_amd_sample.h has the
// sums, the random stream and the draw rule in full; tests/sample_paths_ref.py restates them in Python.
//
// sample_forward_kernel<CAP, HASH>: one wave64 per read, laid out as best_path_forward_kernel -- the column of the
// previous and of the current position in LDS with a hash node -> first slot each; the <= 64 class has one lane per list
// entry, the 400 class loops the column.  Every sum is lse(t_1..t_n) = mx + log(sum exp(t_i - mx)) with the terms added in
// the header's order; a term of -inf adds an exact 0, so list entries that hold no state change no bit and both classes
// return the same values.  A node listed twice holds states at its first entry only.  The hash is asked once per (entry,
// parent): the first-entry slots of the parents in the previous and in the same list go to LDS, the Del levels read them
// there, and they leave with the entry's record.  Every entry leaves one record of 128 bytes (SpRec below).
//
// sample_walk_kernel: one wave per read, lane = sample (hence at most 64 samples).  Each lane carries its own stream
// counter, draws the end state and walks back through the records: per decision the candidate terms are formed once
// into registers (fully unrolled over the 8 parent places, so no array is indexed at run time), then the maximum, the
// weights and the running sums.  The samples of a read mostly stand on the same states, so a wave's record loads fall
// on few addresses; lanes that part only pay the divergence of the decision they part at.  A row is put together in
// registers and stored once; usage counts go out as 32-bit integer atomics.
#pragma once

#include "sparse_dev.h"

namespace phmm {

struct SpParams {  // natural logs, as phmm_params holds them
    double p_mismatch, p_match, p_random, p_end;
    double p_MM, p_IM, p_DM, p_MI, p_II, p_DI, p_MD, p_ID, p_DD;
    int G;  // n_max_gaps
};

static constexpr uint16_t SP_NO_SLOT = 0xffffu;
static constexpr uint32_t SP_IB = 0xffffffffu;  // the walk stands in InsBegin (Begin at column -1)
static constexpr uint32_t SMP_ERR_CAPACITY = 1u, SMP_ERR_WALK = 2u;
static constexpr int SP_DEG = 8, SP_LEVELS = 7;  // degree <= 8 (checked on the host); n_max_gaps <= 6

// What the forward pass leaves per list entry, 128 bytes.  prev[e] / same[e]: the first-entry slot of the parent over the
// node's e-th incoming edge in ASCENDING EDGE INDEX in the previous / the same list, SP_NO_SLOT where the parent is not
// listed (every place of an entry that is a later duplicate, and places e >= degree).  me: the node's own first entry
// in the previous list.  lev[t] is written for t <= G only.
struct alignas(16) SpRec {
    double m, i, d;
    double lev[SP_LEVELS];
    uint16_t prev[SP_DEG], same[SP_DEG];
    uint32_t me, pad0;
    uint64_t pad1;
};
static_assert(sizeof(SpRec) == 128, "record size is part of DESIGN.md and of the chunking");

struct SampleArgs {
    // the model: parents by CSR with edge ids (degree <= 8; the CSR lists a node's edges NEWEST FIRST), init / trans in
    // natural logs as the model was given them
    const uint8_t *emis;
    const uint32_t *par_off, *par_node, *par_edge;
    const double *init_log, *trans_log;
    SpParams lp;
    const uint8_t *bases;
    const uint64_t *read_off;     // [R+1]
    const uint64_t *map_pos_off;  // [total_bases+1]
    const uint32_t *map_nodes;
    const uint32_t *read_ids;     // forward: the reads of this launch's capacity class
    uint64_t ent0;                // first list entry of the chunk: record of entry a is rec[a - ent0]
    SpRec *rec;
    double *ib;                   // InsBegin of column p of the chunk's base g: ib[g - base0]
    uint64_t base0;               // first base of the chunk
    double *logp;                 // [R] ln Z
    double *end_mx, *end_c;       // [R] the maximum and the sum of weights of the end decision
    uint32_t *err;                // [R]
    // walk
    uint32_t r0, r1;              // reads of the chunk
    uint32_t n_samples, n_nodes;
    uint64_t seed;
    uint64_t row0;                // row of base g in plane s: path[(s * plane_rows + g - row0) * stride]
    uint64_t plane_rows;
    uint32_t *path;               // or null
    uint32_t stride;
    double *path_logp;            // [R][S]
    uint32_t *counts;             // [R][S][4]
    uint32_t *usage;              // [S][n_nodes] or null
};

template <int CAP, int HASH> struct SpCol {
    double m[CAP], i[CAP], d[CAP];
    uint32_t id[CAP];
    uint32_t hkey[HASH];
    uint32_t hval[HASH];  // the FIRST slot that lists the node
};
template <int CAP, int HASH> __device__ __forceinline__ int sp_find(const SpCol<CAP, HASH> &c, uint32_t key) {
    uint32_t h = ((key * 2654435761u) >> 16) & (HASH - 1);
    for (;;) {
        const uint32_t k = c.hkey[h];
        if (k == key) return (int)c.hval[h];
        if (k == H_EMPTY) return -1;
        h = (h + 1) & (HASH - 1);
    }
}

// the weight of a term under the maximum mx of its decision (mx finite)
__device__ __forceinline__ double sp_w(double t, double mx) { return t > -INFINITY ? exp(t - mx) : 0.0; }

__device__ __forceinline__ uint64_t sp_mix(uint64_t z) {  // the SplitMix64 finaliser
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static constexpr uint64_t SP_GOLD = 0x9E3779B97F4A7C15ull;
__device__ __forceinline__ double sp_uniform(uint64_t x0, uint64_t d) {
    return (double)(sp_mix(x0 + d * SP_GOLD) >> 11) * 0x1p-53;
}

// The draw rule: t[] holds the log terms in candidate order (-inf: no candidate at that place); returns the choice, -1
// when no term is finite.  t[] is overwritten with the weights.
template <int NC> __device__ __forceinline__ int sp_draw(double (&t)[NC], double u) {
    double mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < NC; i++) mx = fmax(mx, t[i]);
    if (!(mx > -INFINITY)) return -1;
    double c = 0.0;
#pragma unroll
    for (int i = 0; i < NC; i++) {
        t[i] = sp_w(t[i], mx);
        c += t[i];
    }
    const double thr = u * c;
    double run = 0.0;
    int pick = -1, last = -1;
#pragma unroll
    for (int i = 0; i < NC; i++) {
        run += t[i];
        if (pick < 0 && thr < run) pick = i;
        if (t[i] > 0.0) last = i;
    }
    return pick >= 0 ? pick : last;
}

template <int CAP, int HASH>
__global__ void __launch_bounds__(64) sample_forward_kernel(const SampleArgs a) {
    typedef SpCol<CAP, HASH> SCol;
    static_assert(HASH >= 2 * CAP && (HASH & (HASH - 1)) == 0, "hash at half load at most");
    static_assert(CAP < (int)SP_NO_SLOT, "slots are kept in 16 bits");
    __shared__ SCol cols[2];
    __shared__ double lv[2][CAP];  // Del level t - 1 and t
    __shared__ uint16_t sprev[CAP][SP_DEG], ssame[CAP][SP_DEG];
    const int lane = threadIdx.x;
    const uint32_t rd = a.read_ids[blockIdx.x];
    const SpParams &lp = a.lp;
    const uint64_t b0 = a.read_off[rd], len = a.read_off[rd + 1] - b0;
    double ib = -INFINITY;  // InsBegin of the previous column
    int np = 0, cur = 0;
    bool bad = false;
    for (uint64_t pos = 0; pos < len; pos++, cur ^= 1) {
        SCol &C = cols[cur];
        const SCol &P = cols[cur ^ 1];
        const uint64_t e0 = a.map_pos_off[b0 + pos];
        const int n = (int)(a.map_pos_off[b0 + pos + 1] - e0);
        if (n > CAP) {
            bad = true;
            break;
        }
        SpRec *rec = a.rec + (e0 - a.ent0);
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
        // the parents' slots, then Match and Ins from the previous column (column -1: MB = 0, IB = -inf, no node values)
        const double beg_m = pos == 0 ? lp.p_MM : lp.p_IM + ib;
        for (int j = lane; j < n; j += 64) {
            const uint32_t k = C.id[j];
            const bool first = sp_find(C, k) == j;
            const uint32_t p0 = a.par_off[k], deg = first ? a.par_off[k + 1] - p0 : 0u;
            for (uint32_t e = 0; e < (uint32_t)SP_DEG; e++) {
                uint16_t qp = SP_NO_SLOT, qs = SP_NO_SLOT;
                if (e < deg) {
                    const uint32_t u = a.par_node[p0 + deg - 1 - e];  // (ascending edge index)
                    int q = np > 0 ? sp_find(P, u) : -1;
                    if (q >= 0) qp = (uint16_t)q;
                    q = sp_find(C, u);
                    if (q >= 0) qs = (uint16_t)q;
                }
                sprev[j][e] = qp;
                ssame[j][e] = qs;
                rec[j].prev[e] = qp;
                rec[j].same[e] = qs;
            }
            double mv = -INFINITY, iv = -INFINITY;
            uint32_t me = SP_IB;
            if (first) {
                const double beg = a.init_log[k] + beg_m;
                double mx = beg;
                for (uint32_t e = 0; e < deg; e++) {
                    const uint32_t q = sprev[j][e];
                    if (q == SP_NO_SLOT) continue;
                    const double t = a.trans_log[a.par_edge[p0 + deg - 1 - e]];
                    mx = fmax(mx, fmax(t + (lp.p_MM + P.m[q]), fmax(t + (lp.p_IM + P.i[q]), t + (lp.p_DM + P.d[q]))));
                }
                double bv = -INFINITY;
                if (mx > -INFINITY) {
                    double s = 0.0;
                    for (uint32_t e = 0; e < deg; e++) {
                        const uint32_t q = sprev[j][e];
                        if (q == SP_NO_SLOT) continue;
                        const double t = a.trans_log[a.par_edge[p0 + deg - 1 - e]];
                        s += sp_w(t + (lp.p_MM + P.m[q]), mx);
                        s += sp_w(t + (lp.p_IM + P.i[q]), mx);
                        s += sp_w(t + (lp.p_DM + P.d[q]), mx);
                    }
                    s += sp_w(beg, mx);
                    bv = mx + log(s);
                }
                mv = (a.emis[k] == x ? lp.p_match : lp.p_mismatch) + bv;
                const int q = np > 0 ? sp_find(P, k) : -1;
                if (q >= 0) {
                    me = (uint32_t)q;
                    const double t0 = lp.p_MI + P.m[q], t1 = lp.p_II + P.i[q], t2 = lp.p_DI + P.d[q];
                    const double imx = fmax(t0, fmax(t1, t2));
                    if (imx > -INFINITY) iv = lp.p_random + (imx + log((sp_w(t0, imx) + sp_w(t1, imx)) + sp_w(t2, imx)));
                }
            }
            C.m[j] = mv;
            C.i[j] = iv;
            rec[j].m = mv;
            rec[j].i = iv;
            rec[j].me = me;
        }
        // IB of this column (MB of it is -inf)
        ib = lp.p_random + (pos == 0 ? lp.p_MI : lp.p_II + ib);
        if (lane == 0) a.ib[b0 + pos - a.base0] = ib;
        wave_sync();
        // Del level 0 from this column's Match and Ins, and from InsBegin of this column
        const double beg_d = lp.p_ID + ib;
        for (int j = lane; j < n; j += 64) {
            const uint32_t k = C.id[j];
            double v = -INFINITY;
            if (sp_find(C, k) == j) {
                const uint32_t p0 = a.par_off[k], deg = a.par_off[k + 1] - p0;
                const double beg = a.init_log[k] + beg_d;
                double mx = beg;
                for (uint32_t e = 0; e < deg; e++) {
                    const uint32_t q = ssame[j][e];
                    if (q == SP_NO_SLOT) continue;
                    const double t = a.trans_log[a.par_edge[p0 + deg - 1 - e]];
                    mx = fmax(mx, fmax(t + (lp.p_MD + C.m[q]), t + (lp.p_ID + C.i[q])));
                }
                if (mx > -INFINITY) {
                    double s = 0.0;
                    for (uint32_t e = 0; e < deg; e++) {
                        const uint32_t q = ssame[j][e];
                        if (q == SP_NO_SLOT) continue;
                        const double t = a.trans_log[a.par_edge[p0 + deg - 1 - e]];
                        s += sp_w(t + (lp.p_MD + C.m[q]), mx);
                        s += sp_w(t + (lp.p_ID + C.i[q]), mx);
                    }
                    s += sp_w(beg, mx);
                    v = mx + log(s);
                }
            }
            lv[0][j] = v;
            rec[j].lev[0] = v;
        }
        // Del levels 1 .. G: a path through level t comes from level t - 1
        for (int t = 1; t <= lp.G; t++) {
            wave_sync();
            const double *src = lv[(t - 1) & 1];
            double *dst = lv[t & 1];
            for (int j = lane; j < n; j += 64) {
                const uint32_t k = C.id[j];
                double v = -INFINITY;
                if (sp_find(C, k) == j) {
                    const uint32_t p0 = a.par_off[k], deg = a.par_off[k + 1] - p0;
                    double mx = -INFINITY;
                    for (uint32_t e = 0; e < deg; e++) {
                        const uint32_t q = ssame[j][e];
                        if (q == SP_NO_SLOT) continue;
                        mx = fmax(mx, a.trans_log[a.par_edge[p0 + deg - 1 - e]] + (lp.p_DD + src[q]));
                    }
                    if (mx > -INFINITY) {
                        double s = 0.0;
                        for (uint32_t e = 0; e < deg; e++) {
                            const uint32_t q = ssame[j][e];
                            if (q == SP_NO_SLOT) continue;
                            s += sp_w(a.trans_log[a.par_edge[p0 + deg - 1 - e]] + (lp.p_DD + src[q]), mx);
                        }
                        v = mx + log(s);
                    }
                }
                dst[j] = v;
                rec[j].lev[t] = v;
            }
        }
        // D of an entry: the lse of its levels (the lane that owns j wrote them and reads them back)
        for (int j = lane; j < n; j += 64) {
            double mx = -INFINITY;
            for (int t = 0; t <= lp.G; t++) mx = fmax(mx, rec[j].lev[t]);
            double v = -INFINITY;
            if (mx > -INFINITY) {
                double s = 0.0;
                for (int t = 0; t <= lp.G; t++) s += sp_w(rec[j].lev[t], mx);
                v = mx + log(s);
            }
            C.d[j] = v;
            rec[j].d = v;
        }
        wave_sync();
        np = n;
    }
    // ln Z = p_end + lse over the last column in slot order, M, I, D per entry.  The maximum does not round, so it is
    // taken across the lanes; the weights are formed by the lanes and added by lane 0 in slot order, which keeps the sum
    // the same in both capacity classes.  The walk draws the end state against the same maximum and sum.
    double mx = -INFINITY, c = 0.0;
    if (!bad && len > 0) {
        const SCol &L = cols[cur ^ 1];
        SCol &W = cols[cur];
        for (int j = lane; j < np; j += 64) mx = fmax(mx, fmax(L.m[j], fmax(L.i[j], L.d[j])));
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off));
        if (mx > -INFINITY) {
            for (int j = lane; j < np; j += 64) {
                W.m[j] = sp_w(L.m[j], mx);
                W.i[j] = sp_w(L.i[j], mx);
                W.d[j] = sp_w(L.d[j], mx);
            }
            wave_sync();
            if (lane == 0)
                for (int j = 0; j < np; j++) {
                    c += W.m[j];
                    c += W.i[j];
                    c += W.d[j];
                }
        }
    }
    if (lane == 0) {
        a.logp[rd] = bad ? NAN : (mx > -INFINITY ? lp.p_end + (mx + log(c)) : -INFINITY);
        a.end_mx[rd] = mx;
        a.end_c[rd] = c;
        a.err[rd] = bad ? SMP_ERR_CAPACITY : 0u;
    }
}

// One wave per read of the chunk, lane = sample.
__global__ void __launch_bounds__(64) sample_walk_kernel(const SampleArgs a) {
    const uint32_t rd = a.r0 + blockIdx.x, s = threadIdx.x;
    if (s >= a.n_samples) return;
    const SpParams &lp = a.lp;
    const uint64_t b0 = a.read_off[rd], len = a.read_off[rd + 1] - b0;
    const uint32_t stride = a.stride;
    const int G = lp.G;
    uint32_t *plane = a.path ? a.path + ((uint64_t)s * a.plane_rows + (b0 - a.row0)) * stride : nullptr;
    uint32_t *use = a.usage ? a.usage + (uint64_t)s * a.n_nodes : nullptr;
    const double *ibv = a.ib + (b0 - a.base0);
    const double logz = a.logp[rd];
    uint32_t cnt[4] = {0, 0, 0, 0};
    double acc = lp.p_end;
    uint32_t err = 0;
    bool walked = false;
    if (!a.err[rd] && logz > -INFINITY) {
        walked = true;
        const uint64_t x0 = sp_mix(a.seed ^ sp_mix((uint64_t)rd * 64 + s + SP_GOLD));
        uint64_t d = 0;
        // 1. the end state, against the maximum and the sum the forward pass formed
        uint32_t state = SP_IB;
        {
            const uint64_t e0 = a.map_pos_off[b0 + len - 1];
            const uint32_t n = (uint32_t)(a.map_pos_off[b0 + len] - e0);
            const SpRec *rec = a.rec + (e0 - a.ent0);
            const double mx = a.end_mx[rd], thr = sp_uniform(x0, ++d) * a.end_c[rd];
            double run = 0.0;
            uint32_t last = SP_IB;
            for (uint32_t j = 0; j < n && state == SP_IB; j++) {
                const double w[3] = {sp_w(rec[j].m, mx), sp_w(rec[j].i, mx), sp_w(rec[j].d, mx)};
#pragma unroll
                for (uint32_t kd = 0; kd < 3; kd++) {
                    run += w[kd];
                    if (state == SP_IB && thr < run) state = (j << 2) | kd;
                    if (w[kd] > 0.0) last = (j << 2) | kd;
                }
            }
            if (state == SP_IB) state = last;
            if (state == SP_IB) err = SMP_ERR_WALK;
        }
        // state: (slot << 2) | kind of a state of column p, or SP_IB = InsBegin of column p
        for (uint64_t p = len; !err && p-- > 0;) {
            const uint64_t e0 = a.map_pos_off[b0 + p];
            const uint32_t n = (uint32_t)(a.map_pos_off[b0 + p + 1] - e0);
            const SpRec *rec = a.rec + (e0 - a.ent0);
            uint32_t row[8];
#pragma unroll
            for (int c = 0; c < 8; c++) row[c] = 0xffffffffu;
            if (state != SP_IB && (state & 3u) == 2u) {
                // 2. the Del chain of this column: the level, the parents down to level 0, the source of level 0
                uint32_t j = state >> 2;
                if (j >= n) {
                    err = SMP_ERR_WALK;
                    break;
                }
                double tl[SP_LEVELS];
#pragma unroll
                for (int t = 0; t < SP_LEVELS; t++) tl[t] = t <= G ? rec[j].lev[t] : -INFINITY;
                const int T = sp_draw<SP_LEVELS>(tl, sp_uniform(x0, ++d));
                if (T < 0 || (uint32_t)T + 2 > stride) {
                    err = SMP_ERR_WALK;
                    break;
                }
                for (int t = T;; t--) {
                    const uint32_t code = (j << 2) | 2u;
#pragma unroll
                    for (int c = 1; c < 8; c++)
                        if (c == t + 1) row[c] = code;
                    cnt[3]++;
                    const uint32_t k = a.map_nodes[e0 + j];
                    if (use) atomicAdd(&use[k], 1u);
                    const uint32_t p0 = a.par_off[k], deg = a.par_off[k + 1] - p0;
                    uint32_t qs[SP_DEG];
                    double tr[SP_DEG];
#pragma unroll
                    for (int e = 0; e < SP_DEG; e++) {
                        qs[e] = rec[j].same[e];
                        tr[e] = (uint32_t)e < deg && qs[e] != SP_NO_SLOT && qs[e] < n ? a.trans_log[a.par_edge[p0 + deg - 1 - e]] : -INFINITY;
                    }
                    if (t == 0) {
                        double tt[2 * SP_DEG + 1];
#pragma unroll
                        for (int e = 0; e < SP_DEG; e++) {
                            tt[2 * e] = tt[2 * e + 1] = -INFINITY;
                            if (tr[e] > -INFINITY) {
                                tt[2 * e] = tr[e] + (lp.p_MD + rec[qs[e]].m);
                                tt[2 * e + 1] = tr[e] + (lp.p_ID + rec[qs[e]].i);
                            }
                        }
                        tt[2 * SP_DEG] = a.init_log[k] + (lp.p_ID + ibv[p]);
                        const int c = sp_draw<2 * SP_DEG + 1>(tt, sp_uniform(x0, ++d));
                        if (c < 0) err = SMP_ERR_WALK;
                        else if (c == 2 * SP_DEG) {
                            acc += a.init_log[k] + lp.p_ID;
                            state = SP_IB;
                        } else {
#pragma unroll
                            for (int e = 0; e < SP_DEG; e++)
                                if (e == (c >> 1)) {
                                    acc += tr[e] + ((c & 1) ? lp.p_ID : lp.p_MD);
                                    state = (qs[e] << 2) | (uint32_t)(c & 1);
                                }
                        }
                        break;
                    }
                    double tt[SP_DEG];
#pragma unroll
                    for (int e = 0; e < SP_DEG; e++) {
                        double v = -INFINITY;
#pragma unroll
                        for (int u = 0; u < SP_LEVELS - 1; u++)
                            if (u == t - 1 && tr[e] > -INFINITY) v = rec[qs[e]].lev[u];
                        tt[e] = tr[e] > -INFINITY ? tr[e] + (lp.p_DD + v) : -INFINITY;
                    }
                    const int c = sp_draw<SP_DEG>(tt, sp_uniform(x0, ++d));
                    if (c < 0) {
                        err = SMP_ERR_WALK;
                        break;
                    }
#pragma unroll
                    for (int e = 0; e < SP_DEG; e++)
                        if (e == c) {
                            acc += tr[e] + lp.p_DD;
                            j = qs[e];
                        }
                }
                if (err) break;
            }
            // the emitting state of base p and the state it came from
            uint32_t prev = SP_IB;
            if (state == SP_IB) {
                // 5. InsBegin: one predecessor, no draw (InsBegin of column p - 1; at p = 0 it came from Begin)
                row[0] = 0xfffffffdu;  // PHMM_PATH_INS_BEGIN
                cnt[2]++;
                acc += lp.p_random + (p == 0 ? lp.p_MI : lp.p_II);
            } else {
                const uint32_t j = state >> 2;
                if (j >= n) {
                    err = SMP_ERR_WALK;
                    break;
                }
                const uint32_t k = a.map_nodes[e0 + j];
                if (use) atomicAdd(&use[k], 1u);
                row[0] = state;
                const uint64_t pe0 = p > 0 ? a.map_pos_off[b0 + p - 1] : e0;
                const uint32_t pn = p > 0 ? (uint32_t)(e0 - pe0) : 0u;
                const SpRec *prec = a.rec + (pe0 - a.ent0);
                if ((state & 3u) == 0u) {
                    // 3. Match: the parents in the previous list, Begin / InsBegin last
                    const bool hit = a.emis[k] == a.bases[b0 + p];
                    cnt[hit ? 0 : 1]++;
                    acc += hit ? lp.p_match : lp.p_mismatch;
                    const uint32_t p0 = a.par_off[k], deg = a.par_off[k + 1] - p0;
                    uint32_t qp[SP_DEG];
                    double tr[SP_DEG], tt[3 * SP_DEG + 1];
#pragma unroll
                    for (int e = 0; e < SP_DEG; e++) {
                        qp[e] = rec[j].prev[e];
                        tr[e] = (uint32_t)e < deg && qp[e] != SP_NO_SLOT && qp[e] < pn ? a.trans_log[a.par_edge[p0 + deg - 1 - e]] : -INFINITY;
                        tt[3 * e] = tt[3 * e + 1] = tt[3 * e + 2] = -INFINITY;
                        if (tr[e] > -INFINITY) {
                            tt[3 * e] = tr[e] + (lp.p_MM + prec[qp[e]].m);
                            tt[3 * e + 1] = tr[e] + (lp.p_IM + prec[qp[e]].i);
                            tt[3 * e + 2] = tr[e] + (lp.p_DM + prec[qp[e]].d);
                        }
                    }
                    tt[3 * SP_DEG] = a.init_log[k] + (p == 0 ? lp.p_MM : lp.p_IM + ibv[p - 1]);
                    const int c = sp_draw<3 * SP_DEG + 1>(tt, sp_uniform(x0, ++d));
                    if (c < 0) {
                        err = SMP_ERR_WALK;
                        break;
                    }
                    if (c == 3 * SP_DEG) acc += a.init_log[k] + (p == 0 ? lp.p_MM : lp.p_IM);
                    else {
                        const int ce = c / 3, ck = c - 3 * ce;
#pragma unroll
                        for (int e = 0; e < SP_DEG; e++)
                            if (e == ce) {
                                acc += tr[e] + (ck == 0 ? lp.p_MM : ck == 1 ? lp.p_IM : lp.p_DM);
                                prev = (qp[e] << 2) | (uint32_t)ck;
                            }
                    }
                } else {
                    // 4. Ins: M, I, D of the node's first entry in the previous list
                    cnt[2]++;
                    acc += lp.p_random;
                    const uint32_t q = rec[j].me;
                    if (q >= pn) {
                        err = SMP_ERR_WALK;
                        break;
                    }
                    double tt[3] = {lp.p_MI + prec[q].m, lp.p_II + prec[q].i, lp.p_DI + prec[q].d};
                    const int c = sp_draw<3>(tt, sp_uniform(x0, ++d));
                    if (c < 0) {
                        err = SMP_ERR_WALK;
                        break;
                    }
                    acc += c == 0 ? lp.p_MI : c == 1 ? lp.p_II : lp.p_DI;
                    prev = (q << 2) | (uint32_t)c;
                }
            }
            if (plane) {
                uint32_t *out = plane + p * stride;
#pragma unroll
                for (int c = 0; c < 8; c++)
                    if ((uint32_t)c < stride) out[c] = row[c];
            }
            state = prev;
        }
    }
    if (err) atomicMax(&a.err[rd], err);
    const bool ok = walked && !err;
    if (!ok && plane)  // (a walk that failed is reported by the host; a read without a path has all rows PHMM_PATH_NONE)
        for (uint64_t p = 0; p < len; p++)
            for (uint32_t c = 0; c < stride; c++) plane[p * stride + c] = 0xffffffffu;
    const uint64_t o = (uint64_t)rd * a.n_samples + s;
    a.path_logp[o] = ok ? acc : -INFINITY;
    for (int c = 0; c < 4; c++) a.counts[o * 4 + c] = ok ? cnt[c] : 0u;
}

// first list entry of every read (and the total behind the last)
__global__ void __launch_bounds__(256) sample_entry_offsets(const uint64_t *read_off, const uint64_t *map_pos_off,
                                                            uint64_t R, uint64_t *out) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r <= R) out[r] = map_pos_off[read_off[r]];
}

}  // namespace phmm
