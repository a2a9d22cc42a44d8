// Sparse (active-node frontier) kernels: one wave64 per (read[, candidate]).
//
// hinted_score_kernel = PHMMModel::forward_with_mapping_score_only
//   (src/hmmv2/forward.rs:79-89): f_step over mapping.nodes(i) for every read position,
//   non-adaptive, returning table.e of the last position.  It is the inner loop of
//   `infer`: to_full_prob_reads (src/hmmv2/freq.rs:175-192) called once per candidate
//   copy-number vector per iteration (src/multi_dbg/posterior.rs:483-515).  The grid is
//   (reads x candidates): topology, reads and mappings are shared, only init/trans differ.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>

#include "sparse_dyn.h"

namespace phmm {

// a rescale exponent below this in ONE position: see hinted_exact_kernel
static constexpr int HINT_COLLAPSE_EXP = -512;

struct HintedArgs {
    SparseModel M;
    const double *init_c;   // [C][N] linear
    const double *trans_c;  // [C][E] linear
    uint32_t E;
    const uint8_t *bases;
    const uint64_t *read_off;
    const uint64_t *map_pos_off;
    const uint32_t *map_nodes;
    const uint32_t *read_ids;  // reads of this capacity class
    uint64_t R;
    double *out_logp;  // [C][R]
    uint32_t *err;     // [C][R]
    RecPool pool;      // optional (forward_with_mapping, forward.rs:51-75): one record per position, candidate 0 only
};

template <int CAP, int LPN>
__global__ void __launch_bounds__(64) hinted_score_kernel(const HintedArgs a) {
    __shared__ Col<CAP> cols[2];
    __shared__ int16_t lnk_slot[CAP * LPN];
    __shared__ double lnk_w[CAP * LPN];
    __shared__ double dA[CAP], dB[CAP];
    const uint32_t rd = a.read_ids[blockIdx.x];
    const uint32_t cand = blockIdx.y;
    SparseModel M = a.M;
    M.init = a.init_c + (size_t)cand * M.N;
    M.trans = a.trans_c + (size_t)cand * a.E;
    const uint64_t b0 = a.read_off[rd];
    const int len = (int)(a.read_off[rd + 1] - b0);
    uint32_t err = 0;
    if (threadIdx.x == 0) {
        cols[0].n = cols[0].na = 0;
        cols[0].E = 0;
        cols[1].n = cols[1].na = 0;
        cols[1].E = 0;
    }
    wave_sync();
    int pos = 0;
    bool collapse = false;
    for (; pos < len; pos++) {
        const uint64_t o0 = a.map_pos_off[b0 + pos], o1 = a.map_pos_off[b0 + pos + 1];
        const int n = (int)(o1 - o0);
        if (n > CAP) {
            err |= SP_ERR_CAPACITY;
            break;
        }
        err |= fwd_list_step<CAP, LPN>(M, cols[(pos + 1) & 1], cols[pos & 1], a.map_nodes + o0, n, a.bases[b0 + pos],
                                       pos == 0, pos, lnk_slot, lnk_w, dA, dB);
        // a column 2^-512 below the one before it: every listed node died and what is left restarts from an InsBegin
        // chain that is down among the denormals (or below) -- not trusted, see hinted_exact_kernel
        if (pos > 0 && cols[pos & 1].E - cols[(pos + 1) & 1].E < HINT_COLLAPSE_EXP) collapse = true;
        if (a.pool.base && cand == 0 && !store_record_col<CAP>(a.pool, b0 + pos, cols[pos & 1])) err |= SP_ERR_POOL;
    }
    for (int off = 32; off >= 1; off >>= 1) err |= (uint32_t)__shfl_xor((int)err, off);
    const double lp = err ? NAN : (collapse ? -INFINITY : col_log_end(M, cols[(len - 1) & 1]));
    if (threadIdx.x == 0) {
        a.out_logp[(size_t)cand * a.R + rd] = lp;
        a.err[(size_t)cand * a.R + rd] = err;
    }
}

// The same recursion for the <= 64-node class on graphs of degree <= 5 (every DBG), ONE LANE PER LIST ENTRY:
//   * a column lives in registers (m, i, d of the entry on its lane); the LDS only holds two small hashes
//     node -> lane (previous and current list).  Parents' values come by ds_bpermute: the previous column enters
//     through G = p_MM m + p_IM i + p_DM d (one shuffle per parent), the Del levels through the level value;
//   * software-pipelined over the positions: list offsets, node ids, their parent records (ParRec) and init
//     values and the base are requested one or two positions ahead, trans[edge] as soon as the record is there.
// The generic kernel (fwd_list_step) keeps the column in LDS and walks offsets -> ids -> CSR -> edges -> trans:
// ~25 dependent LDS and 5 dependent global round trips per position.  Same sums in the same order.
static constexpr int HL_HASH = 128;
struct HintedLeanShared {
    uint2 ent[2][HL_HASH];  // {node, lane} of the list of position parity
};
__device__ __forceinline__ uint32_t hl_hash(uint32_t id) { return (id * 2654435761u) >> 25; }
__device__ __forceinline__ int hl_find(const uint2 *ent, uint32_t id) {
    uint32_t h = hl_hash(id);
    for (;;) {
        const uint2 e = ent[h];
        if (e.x == id) return (int)e.y;
        if (e.x == 0xffffffffu) return -1;
        h = (h + 1) & (HL_HASH - 1);
    }
}
__device__ __forceinline__ double hl_shfl(double v, int src) { return __shfl(v, src < 0 ? 0 : src); }

// The arithmetic of one list entry, written with explicit roundings (no operand order or fma contraction is left to the
// compiler): hinted_lean_kernel and hinted_packed_kernel<WG, CPL> call these and nothing else on values, so a
// candidate's score has the same bits whichever kernel, group or lane slot evaluated it.
struct HStep {
    // G = p_MM m + p_IM i + p_DM d of the previous column (what flows into Match), H likewise into Ins
    static __device__ __forceinline__ double lin3(double a, double x, double b, double y, double c, double z) {
        return __fma_rn(c, z, __fma_rn(b, y, __dmul_rn(a, x)));
    }
    static __device__ __forceinline__ double acc(double w, double v, double s) { return __fma_rn(w, v, s); }
    // fm: e_k(x) (sum + init c_begin)
    static __device__ __forceinline__ double match(double pe, double sum, double init, double c_begin) {
        return __dmul_rn(pe, __fma_rn(init, c_begin, sum));
    }
    // Del level input p_MD m + p_ID i
    static __device__ __forceinline__ double lv(const LinParams &lp, double m, double i) {
        return __fma_rn(lp.p_ID, i, __dmul_rn(lp.p_MD, m));
    }
    static __device__ __forceinline__ double c_begin(const LinParams &lp, bool first, double ibs) {
        return first ? lp.p_MM : __dmul_rn(lp.p_IM, ibs);
    }
    static __device__ __forceinline__ double ib_cur(const LinParams &lp, bool first, double ibs) {
        return first ? __dmul_rn(lp.p_random, lp.p_MI) : __dmul_rn(__dmul_rn(lp.p_random, lp.p_II), ibs);
    }
    static __device__ __forceinline__ double log_end(const LinParams &lp, double stot, int E) {
        return __fma_rn((double)E, SP_LN2, log(__dmul_rn(lp.p_end, stot)));
    }
};

template <bool PAIRS = false>  // (PAIRS: as in hinted_score_kernel)
__global__ void __launch_bounds__(64) hinted_lean_kernel(const HintedArgs a) {
    constexpr int CAP = 64;
    __shared__ HintedLeanShared sh;
    const int lane = threadIdx.x;
    const uint32_t rd = PAIRS ? a.read_ids[2 * blockIdx.x] : a.read_ids[blockIdx.x];
    const uint32_t cand = PAIRS ? a.read_ids[2 * blockIdx.x + 1] : blockIdx.y;
    const double *init = a.init_c + (size_t)cand * a.M.N;
    const double *trans = a.trans_c + (size_t)cand * a.E;
    const ParRec *prec = a.M.prec;
    const LinParams &lp = a.M.lp;
    const uint64_t b0 = a.read_off[rd];
    const int len = (int)(a.read_off[rd + 1] - b0);
    const uint64_t *po = a.map_pos_off + b0;
    uint32_t err = 0;
    // pipeline: (o, n, id, x) of the current and the next position, records and weights of the current one
    uint64_t o_cur = po[0], o_nx = po[1], o_n2 = po[len >= 2 ? 2 : 1];
    int n_cur = (int)(o_nx - o_cur), n_nx = len >= 2 ? (int)(o_n2 - o_nx) : 0;
    // (inactive lanes read node 0: every load below is unconditional)
    uint32_t id_cur = (lane < n_cur && n_cur <= CAP) ? a.map_nodes[o_cur + lane] : 0u;
    uint32_t id_nx = (lane < n_nx && n_nx <= CAP) ? a.map_nodes[o_nx + lane] : 0u;
    ParRec rc_cur = prec[id_cur];
    double in_cur = init[id_cur];
    double w_cur[ADJ_DEG];
#pragma unroll
    for (int q = 0; q < ADJ_DEG; q++) w_cur[q] = q < (int)rc_cur.npar ? trans[rc_cur.pedge[q]] : 0.0;
    uint8_t x_cur = a.bases[b0], x_nx = len >= 2 ? a.bases[b0 + 1] : (uint8_t)0;
    // previous column on the lanes of ITS list order
    double pm = 0.0, pi = 0.0, pd = 0.0, m = 0.0, ii = 0.0, d = 0.0, ibs = 0.0;
    int Eprev = 0, n_prev = 0;
    bool collapse = false;
#ifdef PHMM_LEAN_PROF
    long long pt[8] = {0, 0, 0, 0, 0, 0, 0, 0}, pc0 = 0;
#define HPROF(k)                          \
    {                                     \
        const long long now_ = clock64(); \
        pt[k] += now_ - pc0;              \
        pc0 = now_;                       \
    }
#else
#define HPROF(k)
#endif
    for (int pos = 0; pos < len; pos++) {
        if (n_cur > CAP) {
            err |= SP_ERR_CAPACITY;
            break;
        }
#ifdef PHMM_LEAN_PROF
        pc0 = clock64();
#endif
        // ---- requests for the positions ahead
        const ParRec rc_nx = prec[id_nx];
        const double in_nx = init[id_nx];
        const uint64_t o_n3 = po[pos + 3 <= len ? pos + 3 : len];
        const int n_n2 = pos + 2 < len ? (int)(o_n3 - o_n2) : 0;
        const uint32_t id_n2 = (lane < n_n2 && n_n2 <= CAP) ? a.map_nodes[o_n2 + lane] : 0u;
        const uint8_t x_n2 = pos + 2 < len ? a.bases[b0 + pos + 2] : (uint8_t)0;
        HPROF(0)
        // ---- hash of this position's list
        const bool first = pos == 0;
        const int n = n_cur;
        const bool has = lane < n;
        uint2 *hc = sh.ent[pos & 1];
        const uint2 *hp = sh.ent[(pos + 1) & 1];
        for (int h = lane; h < HL_HASH; h += 64) hc[h].x = 0xffffffffu;
        wave_sync();
        if (has) {
            uint32_t h = hl_hash(id_cur);
            for (;;) {
                const uint32_t old = atomicCAS(&hc[h].x, 0xffffffffu, id_cur);
                if (old == 0xffffffffu) break;
                if (old == id_cur) {
                    err |= SP_ERR_DUPLICATE;
                    break;
                }
                h = (h + 1) & (HL_HASH - 1);
            }
            hc[h].y = (uint32_t)lane;
        }
        wave_sync();
        HPROF(1)
        // ---- fm, fi (forward.rs:337-388), fib (541-545)
        // (InsBegin of the previous column in that column's scale, fib forward.rs:541-545: carried along with the
        // exact power-of-two rescales instead of exp(logib[pos-1] - E ln 2) per position)
        const double c_begin = HStep::c_begin(lp, first, ibs);
        const double ib_cur = HStep::ib_cur(lp, first, ibs);
        const double c_del = __dmul_rn(lp.p_ID, ib_cur);
        const bool hadp = lane < n_prev;
        const double G = hadp ? HStep::lin3(lp.p_MM, pm, lp.p_IM, pi, lp.p_DM, pd) : 0.0;
        const double H = hadp ? HStep::lin3(lp.p_MI, pm, lp.p_II, pi, lp.p_DI, pd) : 0.0;
        int ps[ADJ_DEG], cs[ADJ_DEG];
        uint32_t anyq = 0;  // wave-uniform: some lane has a q-th parent (on a DBG mostly q = 0 only)
#pragma unroll
        for (int q = 0; q < ADJ_DEG; q++) {
            const bool use = has && q < (int)rc_cur.npar && w_cur[q] != 0.0;
            ps[q] = cs[q] = -1;
            if (__ballot(use) != 0ull) {
                anyq |= 1u << q;
                ps[q] = (use && !first) ? hl_find(hp, rc_cur.par[q]) : -1;
                cs[q] = use ? hl_find(hc, rc_cur.par[q]) : -1;
            }
        }
        const int os = (has && !first) ? hl_find(hp, id_cur) : -1;
        HPROF(2)
        double acc = 0.0;
#pragma unroll
        for (int q = 0; q < ADJ_DEG; q++) {
            if (!(anyq & (1u << q))) continue;
            const double v = hl_shfl(G, ps[q]);
            if (ps[q] >= 0) acc = HStep::acc(w_cur[q], v, acc);
        }
        const double hv = hl_shfl(H, os);
        m = ii = d = 0.0;
        if (has) {
            const double pe = rc_cur.emis == x_cur ? lp.p_match : lp.p_mismatch;
            m = HStep::match(pe, acc, in_cur, c_begin);
            ii = os >= 0 ? __dmul_rn(lp.p_random, hv) : 0.0;
        }
        HPROF(3)
        // ---- fd0 + n_max_gaps x fdt restricted to the list (forward.rs:423-524)
        double lv = HStep::lv(lp, m, ii);
        for (int t = 0; t <= lp.n_max_gaps; t++) {
            double sacc = 0.0;
#pragma unroll
            for (int q = 0; q < ADJ_DEG; q++) {
                if (!(anyq & (1u << q))) continue;
                const double v = hl_shfl(lv, cs[q]);
                if (cs[q] >= 0) sacc = HStep::acc(w_cur[q], v, sacc);
            }
            if (t == 0) sacc = __fma_rn(in_cur, c_del, sacc);
            else sacc = __dmul_rn(sacc, lp.p_DD);
            sacc = has ? sacc : 0.0;
            d = __dadd_rn(d, sacc);
            lv = sacc;
        }
        HPROF(4)
        // ---- rescale so that the column maximum is in [0.5, 1)
        const double mx = wave_max(fmax(has ? fmax(fmax(m, ii), d) : 0.0, ib_cur));
        const int e = sp_exp_of(mx);
        collapse |= !first && e < HINT_COLLAPSE_EXP;
        const double sc = sp_pow2(-e);
        m = __dmul_rn(m, sc);
        ii = __dmul_rn(ii, sc);
        d = __dmul_rn(d, sc);
        const int Ecur = (first ? 0 : Eprev) + e;
        ibs = __dmul_rn(ib_cur, sc);
        if (a.pool.base && cand == 0) {
            // forward record of the position (every entry carries m, i and d)
            const uint64_t idb = (uint64_t)((n + 1) & ~1) * 4;
            const uint64_t bytes = 16 + idb + (uint64_t)(3 * n) * 8;
            const uint64_t o = pool_alloc(a.pool, bytes);
            if (o + bytes > a.pool.cap) err |= SP_ERR_POOL;
            else {
                uint8_t *rec = a.pool.base + o;
                if (lane == 0) {
                    ((uint32_t *)rec)[0] = (uint32_t)n;
                    ((uint32_t *)rec)[1] = (uint32_t)n;
                    ((int *)rec)[2] = Ecur;
                    ((uint32_t *)rec)[3] = 0;
                    a.pool.off[b0 + pos] = o + 8;
                }
                if (has) {
                    ((uint32_t *)(rec + 16))[lane] = id_cur;
                    double *om = (double *)(rec + 16 + idb);
                    om[lane] = m;
                    om[n + lane] = ii;
                    om[2 * n + lane] = d;
                }
            }
        }
        HPROF(5)
        // ---- the column becomes the previous one; weights of the next position (its record has arrived)
        pm = m;
        pi = ii;
        pd = d;
        Eprev = Ecur;
        n_prev = n;
#pragma unroll
        for (int q = 0; q < ADJ_DEG; q++) w_cur[q] = q < (int)rc_nx.npar ? trans[rc_nx.pedge[q]] : 0.0;
        o_cur = o_nx;
        o_nx = o_n2;
        o_n2 = o_n3;
        n_cur = n_nx;
        n_nx = n_n2;
        id_cur = id_nx;
        id_nx = id_n2;
        rc_cur = rc_nx;
        in_cur = in_nx;
        x_cur = x_nx;
        x_nx = x_n2;
        HPROF(6)
    }
#ifdef PHMM_LEAN_PROF
    if (blockIdx.x == 0 && blockIdx.y == 0 && lane == 0 && len > 0)
        printf("hinted_lean prof: len %d | requests %lld hash %lld exp+lookups %lld fm %lld del %lld rescale+store %lld rotate+weights %lld (cycles/step)\n",
               len, pt[0] / len, pt[1] / len, pt[2] / len, pt[3] / len, pt[4] / len, pt[5] / len, pt[6] / len);
#endif
    for (int off = 32; off >= 1; off >>= 1) err |= (uint32_t)__shfl_xor((int)err, off);
    // fe (forward.rs:554-558) of the last column
    const double stot = wave_sum(lane < n_prev ? __dadd_rn(__dadd_rn(pm, pi), pd) : 0.0);
    const double lpv = err ? NAN : (collapse ? -INFINITY : HStep::log_end(lp, stot, Eprev));
    if (lane == 0) {
        a.out_logp[(size_t)cand * a.R + rd] = lpv;
        a.err[(size_t)cand * a.R + rd] = err;
    }
}

// ---------------------------------------------------------------- candidate batches: several candidates per wave
// The loop of sample_posterior_once (multi_dbg/posterior.rs:483-515) runs the SAME reads over the SAME lists for
// every candidate copy-number vector; only init / trans differ.  A mapping list holds ~5 nodes (cfg3: 98.9 % of
// the positions <= 8, all but 3e-5 <= 16), so one lane per list entry leaves 9 lanes in 10 idle, and a wave per
// (read, candidate) repeats the whole topology walk -- list, hash, parent lookups -- per candidate.  Here a wave
// owns one read and G = 64 / WG candidates: lane = (candidate group, list slot), slots < WG.  The list, its hash
// and the parent / own-previous lookups are done once per position for all groups; per candidate only init[node],
// trans[edge] and the arithmetic differ; reductions (column maximum, end sum) are segmented over the WG lanes of a
// group.  Reads whose longest list exceeds WG take the next class (16, 32, then the one-candidate kernels).
// Same sums in the same order as hinted_lean_kernel: bit-equal results.
// maximum of NON-NEGATIVE values over the WG lanes of a group, in every lane, on the DPP path (VALU moves, no LDS
// round trips -- the kernel is VALU-issue bound, profiles/r2_candidates64_sq_counters.txt, and a __shfl_xor of a
// double is two ds_bpermute plus their address arithmetic): quad permutes and the half-row mirror for 8 lanes, row
// rotations for a row of 16, one cross-row shuffle on top for 32.
template <int WG> __device__ __forceinline__ double group_max(double v) {
    static_assert(WG == 8 || WG == 16 || WG == 32, "group width");
    if (WG == 8) {
        v = fmax(v, dpp_d<0xB1, 0xf>(0.0, v));   // quad_perm [1,0,3,2]
        v = fmax(v, dpp_d<0x4E, 0xf>(0.0, v));   // quad_perm [2,3,0,1]
        v = fmax(v, dpp_d<0x141, 0xf>(0.0, v));  // row_half_mirror: the other quad of the 8
        return v;
    }
    v = fmax(v, dpp_d<0x128, 0xf>(0.0, v));  // row_ror 8, 4, 2, 1
    v = fmax(v, dpp_d<0x124, 0xf>(0.0, v));
    v = fmax(v, dpp_d<0x122, 0xf>(0.0, v));
    v = fmax(v, dpp_d<0x121, 0xf>(0.0, v));
    if (WG == 32) v = fmax(v, __shfl_xor(v, 16));
    return v;
}
// Sum over the WG lanes of a group in the association of wave_sum (sparse_dev.h: an inclusive Hillis-Steele scan read
// at the last lane) restricted to the group -- lanes beyond a list are zeros there and here, so a candidate's end
// sum has the same bits whether its list sat alone on a wave or in a group.
template <int WG> __device__ __forceinline__ double group_sum(double v, int slot) {
#pragma unroll
    for (int off = 1; off < WG; off <<= 1) {
        const double t = __shfl_up(v, off, WG);
        v += slot >= off ? t : 0.0;
    }
    return __shfl(v, WG - 1, WG);
}

// PAIRS (phmm_full_prob_reads_copy_num_changes): a wave takes its read and its G x CPL candidates from a work unit of
// read_ids, {read, candidate of (group, c) at 1 + group * CPL + c}, 0xffffffff for an idle slot (which computes a
// copy of the unit's first candidate and writes nothing), instead of a read and blockIdx.y.
template <int WG, int CPL, bool PAIRS = false>
__global__ void __launch_bounds__(64) hinted_packed_kernel(const HintedArgs a, const uint32_t n_cand) {
    // CPL candidates per lane on top of the G = 64 / WG candidate groups of a wave: the topology work of a position
    // (list, records, hash, lookups: ~100 VALU wave-instructions) is shared by G x CPL candidates, whose own work
    // (~70 each: weights, G / H, shuffles, Del levels, rescale) runs CPL times per lane.
    constexpr int G = 64 / WG;
    __shared__ HintedLeanShared sh;
    const int lane = threadIdx.x;
    const int slot = lane % WG, grp = lane / WG, gbase = grp * WG;
    const uint32_t *unit = a.read_ids + (size_t)blockIdx.x * (1 + G * CPL);
    const uint32_t rd = PAIRS ? unit[0] : a.read_ids[blockIdx.x];
    uint32_t cand[CPL];
    bool cand_ok[CPL];
    const double *init[CPL], *trans[CPL];
#pragma unroll
    for (int c = 0; c < CPL; c++) {
        if (PAIRS) {
            cand[c] = unit[1 + grp * CPL + c];
            cand_ok[c] = cand[c] != 0xffffffffu;
            if (!cand_ok[c]) cand[c] = unit[1];
        } else {
            cand[c] = (blockIdx.y * G + (uint32_t)grp) * CPL + c;
            cand_ok[c] = cand[c] < n_cand;
            if (!cand_ok[c]) cand[c] = n_cand - 1;  // (idle slots of the last wave compute a copy; nothing is written)
        }
        init[c] = a.init_c + (size_t)cand[c] * a.M.N;
        trans[c] = a.trans_c + (size_t)cand[c] * a.E;
    }
    const ParRec *prec = a.M.prec;
    const LinParams &lp = a.M.lp;
    const uint64_t b0 = a.read_off[rd];
    const int len = (int)(a.read_off[rd + 1] - b0);
    const uint64_t *po = a.map_pos_off + b0;
    uint32_t err = 0;
    uint64_t o_cur = po[0], o_nx = po[1], o_n2 = po[len >= 2 ? 2 : 1];
    int n_cur = (int)(o_nx - o_cur), n_nx = len >= 2 ? (int)(o_n2 - o_nx) : 0;
    uint32_t id_cur = (slot < n_cur && n_cur <= WG) ? a.map_nodes[o_cur + slot] : 0u;
    uint32_t id_nx = (slot < n_nx && n_nx <= WG) ? a.map_nodes[o_nx + slot] : 0u;
    ParRec rc_cur = prec[id_cur];
    double in_cur[CPL], w_cur[CPL][ADJ_DEG];
#pragma unroll
    for (int c = 0; c < CPL; c++) {
        in_cur[c] = init[c][id_cur];
#pragma unroll
        for (int q = 0; q < ADJ_DEG; q++) w_cur[c][q] = q < (int)rc_cur.npar ? trans[c][rc_cur.pedge[q]] : 0.0;
    }
    uint8_t x_cur = a.bases[b0], x_nx = len >= 2 ? a.bases[b0 + 1] : (uint8_t)0;
    double pm[CPL], pi[CPL], pd[CPL], ibs[CPL];
    int Eprev[CPL];
    bool collapse[CPL];
#pragma unroll
    for (int c = 0; c < CPL; c++) {
        pm[c] = pi[c] = pd[c] = ibs[c] = 0.0;
        Eprev[c] = 0;
        collapse[c] = false;
    }
    int n_prev = 0;
    for (int pos = 0; pos < len; pos++) {
        if (n_cur > WG) {
            err |= SP_ERR_CAPACITY;
            break;
        }
        // ---- requests for the positions ahead
        const ParRec rc_nx = prec[id_nx];
        double in_nx[CPL];
#pragma unroll
        for (int c = 0; c < CPL; c++) in_nx[c] = init[c][id_nx];
        const uint64_t o_n3 = po[pos + 3 <= len ? pos + 3 : len];
        const int n_n2 = pos + 2 < len ? (int)(o_n3 - o_n2) : 0;
        const uint32_t id_n2 = (slot < n_n2 && n_n2 <= WG) ? a.map_nodes[o_n2 + slot] : 0u;
        const uint8_t x_n2 = pos + 2 < len ? a.bases[b0 + pos + 2] : (uint8_t)0;
        // ---- hash of this position's list: node -> slot (group 0 inserts; every group reads)
        const bool first = pos == 0;
        const int n = n_cur;
        const bool has = slot < n;
        uint2 *hc = sh.ent[pos & 1];
        const uint2 *hp = sh.ent[(pos + 1) & 1];
        for (int h = lane; h < HL_HASH; h += 64) hc[h].x = 0xffffffffu;
        wave_sync();
        if (has && grp == 0) {
            uint32_t h = hl_hash(id_cur);
            for (;;) {
                const uint32_t old = atomicCAS(&hc[h].x, 0xffffffffu, id_cur);
                if (old == 0xffffffffu) break;
                if (old == id_cur) {
                    err |= SP_ERR_DUPLICATE;
                    break;
                }
                h = (h + 1) & (HL_HASH - 1);
            }
            hc[h].y = (uint32_t)slot;
        }
        wave_sync();
        // ---- the topology of the position, once for every candidate of the wave: lanes of the in-list parents in the
        // previous (ps) and the current (cs) list, own lane in the previous list (os)
        const bool hadp = slot < n_prev;
        int ps[ADJ_DEG], cs[ADJ_DEG];
        uint32_t anyq = 0;  // wave-uniform: some lane has a q-th parent (on a DBG mostly q = 0 only)
#pragma unroll
        for (int q = 0; q < ADJ_DEG; q++) {
            // (the topology test only: a candidate whose weight is 0 multiplies by it -- the one-candidate kernel
            // skips such a parent, which adds the same +0.0)
            const bool use = has && q < (int)rc_cur.npar;
            ps[q] = cs[q] = -1;
            if (__ballot(use) != 0ull) {
                anyq |= 1u << q;
                ps[q] = (use && !first) ? hl_find(hp, rc_cur.par[q]) : -1;
                cs[q] = use ? hl_find(hc, rc_cur.par[q]) : -1;
            }
        }
        const int os = (has && !first) ? hl_find(hp, id_cur) : -1;
        const double pe = rc_cur.emis == x_cur ? lp.p_match : lp.p_mismatch;
        // byte addresses of the shuffles (ds_bpermute), once for all candidates of the lane
        int aps[ADJ_DEG], acs[ADJ_DEG];
#pragma unroll
        for (int q = 0; q < ADJ_DEG; q++) {
            aps[q] = (gbase + (ps[q] < 0 ? 0 : ps[q])) << 2;
            acs[q] = (gbase + (cs[q] < 0 ? 0 : cs[q])) << 2;
        }
        const int aos = (gbase + (os < 0 ? 0 : os)) << 2;
        auto pull = [](int addr, double v) -> double {
            const long long b = __double_as_longlong(v);
            const int lo = __builtin_amdgcn_ds_bpermute(addr, (int)(b & 0xffffffffll));
            const int hi = __builtin_amdgcn_ds_bpermute(addr, (int)(b >> 32));
            return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned int)lo);
        };
        // ---- per candidate: fm, fi (forward.rs:337-388), fib (541-545), fd0 + n_max_gaps x fdt restricted to the list
        // (forward.rs:423-524), rescale.  Branch-free: a parent that is not in the list (or whose edge has weight 0 for
        // this candidate) enters with weight 0 -- fma(0, v, s) = s exactly, what skipping it gives.
#pragma unroll
        for (int c = 0; c < CPL; c++) {
            const double c_begin = HStep::c_begin(lp, first, ibs[c]);
            const double ib_cur = HStep::ib_cur(lp, first, ibs[c]);
            const double c_del = __dmul_rn(lp.p_ID, ib_cur);
            const double Gv = hadp ? HStep::lin3(lp.p_MM, pm[c], lp.p_IM, pi[c], lp.p_DM, pd[c]) : 0.0;
            const double Hv = hadp ? HStep::lin3(lp.p_MI, pm[c], lp.p_II, pi[c], lp.p_DI, pd[c]) : 0.0;
            const double hv = pull(aos, Hv);
            double m, ii, d = 0.0;
            if (anyq <= 1u) {
                // the common case on a DBG: at most one in-list parent per entry
                const double wp = ps[0] >= 0 ? w_cur[c][0] : 0.0, wc = cs[0] >= 0 ? w_cur[c][0] : 0.0;
                const double acc = HStep::acc(wp, pull(aps[0], Gv), 0.0);
                m = has ? HStep::match(pe, acc, in_cur[c], c_begin) : 0.0;
                ii = (has && os >= 0) ? __dmul_rn(lp.p_random, hv) : 0.0;
                double lv = HStep::lv(lp, m, ii);
                for (int t = 0; t <= lp.n_max_gaps; t++) {
                    double sacc = HStep::acc(wc, pull(acs[0], lv), 0.0);
                    sacc = t == 0 ? __fma_rn(in_cur[c], c_del, sacc) : __dmul_rn(sacc, lp.p_DD);
                    sacc = has ? sacc : 0.0;
                    d = __dadd_rn(d, sacc);
                    lv = sacc;
                }
            } else {
                double wp[ADJ_DEG], wc[ADJ_DEG];
#pragma unroll
                for (int q = 0; q < ADJ_DEG; q++) {
                    wp[q] = ps[q] >= 0 ? w_cur[c][q] : 0.0;
                    wc[q] = cs[q] >= 0 ? w_cur[c][q] : 0.0;
                }
                double acc = 0.0;
#pragma unroll
                for (int q = 0; q < ADJ_DEG; q++)
                    if (anyq & (1u << q)) acc = HStep::acc(wp[q], pull(aps[q], Gv), acc);
                m = has ? HStep::match(pe, acc, in_cur[c], c_begin) : 0.0;
                ii = (has && os >= 0) ? __dmul_rn(lp.p_random, hv) : 0.0;
                double lv = HStep::lv(lp, m, ii);
                for (int t = 0; t <= lp.n_max_gaps; t++) {
                    double sacc = 0.0;
#pragma unroll
                    for (int q = 0; q < ADJ_DEG; q++)
                        if (anyq & (1u << q)) sacc = HStep::acc(wc[q], pull(acs[q], lv), sacc);
                    sacc = t == 0 ? __fma_rn(in_cur[c], c_del, sacc) : __dmul_rn(sacc, lp.p_DD);
                    sacc = has ? sacc : 0.0;
                    d = __dadd_rn(d, sacc);
                    lv = sacc;
                }
            }
            // rescale so that the column maximum of THIS candidate is in [0.5, 1)
            const double mx = group_max<WG>(fmax(fmax(fmax(m, ii), d), ib_cur));
            const int e = sp_exp_of(mx);
            collapse[c] |= !first && e < HINT_COLLAPSE_EXP;
            const double sc = sp_pow2(-e);
            pm[c] = __dmul_rn(m, sc);
            pi[c] = __dmul_rn(ii, sc);
            pd[c] = __dmul_rn(d, sc);
            Eprev[c] = (first ? 0 : Eprev[c]) + e;
            ibs[c] = __dmul_rn(ib_cur, sc);
        }
        // ---- the column becomes the previous one; weights of the next position (its record has arrived)
        n_prev = n;
        {
            // (edge weights only for parent slots some lane of the wave uses: mostly the first)
            int npmax = (int)rc_nx.npar;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) npmax = max(npmax, __shfl_xor(npmax, off));
            npmax = __builtin_amdgcn_readfirstlane(npmax);
#pragma unroll
            for (int c = 0; c < CPL; c++) {
#pragma unroll
                for (int q = 0; q < ADJ_DEG; q++) {
                    if (q < npmax) w_cur[c][q] = q < (int)rc_nx.npar ? trans[c][rc_nx.pedge[q]] : 0.0;
                    else w_cur[c][q] = 0.0;
                }
                in_cur[c] = in_nx[c];
            }
        }
        o_cur = o_nx;
        o_nx = o_n2;
        o_n2 = o_n3;
        n_cur = n_nx;
        n_nx = n_n2;
        id_cur = id_nx;
        id_nx = id_n2;
        rc_cur = rc_nx;
        x_cur = x_nx;
        x_nx = x_n2;
    }
    for (int off = 32; off >= 1; off >>= 1) err |= (uint32_t)__shfl_xor((int)err, off);
    // fe (forward.rs:554-558) of the last column, per candidate
#pragma unroll
    for (int c = 0; c < CPL; c++) {
        const double stot = group_sum<WG>(slot < n_prev ? __dadd_rn(__dadd_rn(pm[c], pi[c]), pd[c]) : 0.0, slot);
        const double lpv = err ? NAN : (collapse[c] ? -INFINITY : HStep::log_end(lp, stot, Eprev[c]));
        if (slot == 0 && cand_ok[c]) {
            a.out_logp[(size_t)cand[c] * a.R + rd] = lpv;
            a.err[(size_t)cand[c] * a.R + rd] = err;
        }
    }
}

}  // namespace phmm

#include "hinted_wide_kernel.h"

namespace phmm {

// ---- wide-range fallback of the hinted forward -----------------------------------------------------------
// forward_with_mappings (forward.rs:79-89, 276-306, 337-388, 423-524, 541-558: fm, fi, fib, fd0 + n_max_gaps x fdt
// over the position's list, fe at the end) with EVERY value carrying its own binary exponent -- a double mantissa
// in [0.5, 1) and an int exponent -- so that nothing underflows whatever its distance from the column's best value:
// the range of the reference's natural-log f64 with plain multiply-adds instead of a log-sum-exp per term.  One
// wave per (candidate, read).  It runs for the pairs the scaled kernels returned -inf for.  That happens when every
// node of a read's lists dies -- a candidate that sets a k-mer on the read's path to copy number 0 -- hundreds of
// positions into the read: the reference then still holds the InsBegin chain (p_random * p_II per base, never
// zero), which re-enters the graph behind the cut, and returns a finite ln P of about -7 per base of the cut-off
// prefix.  In the scaled linear domain (ONE exponent per column) that chain is 2^-1075 below the read's own path
// after ~105 bases and is gone, so the restart is lost; here it is not.
struct XF {
    double m;  // 0, or in [0.5, 1)
    int e;
};
__device__ __forceinline__ XF xf_norm(double v, int e) {
    if (v == 0.0) return XF{0.0, 0};
    int k;
    const double m = frexp(v, &k);
    return XF{m, e + k};
}
__device__ __forceinline__ XF xf_from(double p) { return xf_norm(p, 0); }
__device__ __forceinline__ XF xf_mul(XF a, double p) { return xf_norm(a.m * p, a.e); }
__device__ __forceinline__ XF xf_mulx(XF a, XF b) { return xf_norm(a.m * b.m, a.e + b.e); }
__device__ __forceinline__ XF xf_add(XF a, XF b) {
    if (a.m == 0.0) return b;
    if (b.m == 0.0) return a;
    if (a.e < b.e) {
        const XF t = a;
        a = b;
        b = t;
    }
    const int d = b.e - a.e;
    if (d < -1000) return a;
    return xf_norm(a.m + ldexp(b.m, d), a.e);
}
__device__ __forceinline__ double xf_log(XF a) { return a.m == 0.0 ? -INFINITY : log(a.m) + (double)a.e * SP_LN2; }

// (two sizes: lists of up to 64 nodes -- nearly every read -- keep 9 KB of LDS per wave, so that thousands of pairs
// run at once; the full 400-slot version holds 46 KB)
template <int XCAP, int XHASH> struct ExactCol {
    uint32_t id[XCAP];
    double m[XCAP], i[XCAP], d[XCAP];
    int me[XCAP], ie[XCAP], de[XCAP];
    uint32_t hkey[XHASH];
    uint16_t hval[XHASH];
};
template <int XCAP, int XHASH> __device__ __forceinline__ int xl_find(const ExactCol<XCAP, XHASH> &c, uint32_t key) {
    uint32_t h = ((key * 2654435761u) >> 16) & (XHASH - 1);
    for (;;) {
        const uint32_t k = c.hkey[h];
        if (k == key) return (int)c.hval[h];
        if (k == 0xffffffffu) return -1;
        h = (h + 1) & (XHASH - 1);
    }
}
template <int XCAP, int XHASH>
__global__ void __launch_bounds__(64) hinted_exact_kernel(const HintedArgs a, const uint2 *pairs, double *res) {
    typedef ExactCol<XCAP, XHASH> XCol;
    __shared__ XCol cols[2];
    __shared__ double ta[XCAP], tb[XCAP];
    __shared__ int tae[XCAP], tbe[XCAP];
    const int lane = threadIdx.x;
    const uint32_t cand = pairs[blockIdx.x].x, rd = pairs[blockIdx.x].y;
    const double *init = a.init_c + (size_t)cand * a.M.N;
    const double *trans = a.trans_c + (size_t)cand * a.E;
    const LinParams &lp = a.M.lp;
    const uint64_t b0 = a.read_off[rd], len = a.read_off[rd + 1] - b0;
    XF mb = xf_from(1.0), ib = XF{0.0, 0};  // f_init (forward.rs:255-266)
    int np = 0, cur = 0;
    bool bad = false;
    for (uint64_t pos = 0; pos < len; pos++, cur ^= 1) {
        XCol &C = cols[cur];
        const XCol &P = cols[cur ^ 1];
        const uint64_t e0 = a.map_pos_off[b0 + pos];
        const int n = (int)(a.map_pos_off[b0 + pos + 1] - e0);
        if (n > XCAP) {
            bad = true;
            break;
        }
        const uint8_t x = a.bases[b0 + pos];
        for (int h = lane; h < XHASH; h += 64) C.hkey[h] = 0xffffffffu;
        wave_sync();
        for (int j = lane; j < n; j += 64) {
            const uint32_t k = a.map_nodes[e0 + j];
            C.id[j] = k;
            uint32_t h = ((k * 2654435761u) >> 16) & (XHASH - 1);
            for (;;) {
                const uint32_t old = atomicCAS(&C.hkey[h], 0xffffffffu, k);
                if (old == 0xffffffffu) {
                    C.hval[h] = (uint16_t)j;
                    break;
                }
                if (old == k) break;  // (a node listed twice: the first entry stands)
                h = (h + 1) & (XHASH - 1);
            }
        }
        wave_sync();
        // fm, fi from the previous column (empty at pos 0)
        const XF beg_m = xf_add(xf_mul(mb, lp.p_MM), xf_mul(ib, lp.p_IM));
        for (int j = lane; j < n; j += 64) {
            const uint32_t k = C.id[j];
            XF from_normal{0.0, 0};
            for (uint32_t e = a.M.par_off[k]; e < a.M.par_off[k + 1]; e++) {
                const int q = np > 0 ? xl_find(P, a.M.par_node[e]) : -1;
                if (q < 0) continue;
                const XF inner = xf_add(xf_add(xf_mul(XF{P.m[q], P.me[q]}, lp.p_MM), xf_mul(XF{P.i[q], P.ie[q]}, lp.p_IM)),
                                        xf_mul(XF{P.d[q], P.de[q]}, lp.p_DM));
                from_normal = xf_add(from_normal, xf_mul(inner, trans[a.M.par_edge[e]]));
            }
            const XF mv = xf_mul(xf_add(from_normal, xf_mul(beg_m, init[k])), a.M.emis[k] == x ? lp.p_match : lp.p_mismatch);
            C.m[j] = mv.m;
            C.me[j] = mv.e;
            const int me = np > 0 ? xl_find(P, k) : -1;
            XF iv{0.0, 0};
            if (me >= 0)
                iv = xf_mul(xf_add(xf_add(xf_mul(XF{P.m[me], P.me[me]}, lp.p_MI), xf_mul(XF{P.i[me], P.ie[me]}, lp.p_II)),
                                   xf_mul(XF{P.d[me], P.de[me]}, lp.p_DI)),
                            lp.p_random);
            C.i[j] = iv.m;
            C.ie[j] = iv.e;
        }
        ib = xf_mul(xf_add(xf_mul(mb, lp.p_MI), xf_mul(ib, lp.p_II)), lp.p_random);  // fib; fmb = 0
        mb = XF{0.0, 0};
        wave_sync();
        // fd0 from this column's m, i; then the Del levels over the same list
        const XF beg_d = xf_mul(ib, lp.p_ID);  // (mb = 0)
        for (int j = lane; j < n; j += 64) {
            const uint32_t k = C.id[j];
            XF from_normal{0.0, 0};
            for (uint32_t e = a.M.par_off[k]; e < a.M.par_off[k + 1]; e++) {
                const int q = xl_find(C, a.M.par_node[e]);
                if (q < 0) continue;
                const XF g = xf_add(xf_mul(XF{C.m[q], C.me[q]}, lp.p_MD), xf_mul(XF{C.i[q], C.ie[q]}, lp.p_ID));
                from_normal = xf_add(from_normal, xf_mul(g, trans[a.M.par_edge[e]]));
            }
            const XF v = xf_add(from_normal, xf_mul(beg_d, init[k]));
            ta[j] = v.m;
            tae[j] = v.e;
            C.d[j] = v.m;
            C.de[j] = v.e;
        }
        double *src = ta, *dst = tb;
        int *srce = tae, *dste = tbe;
        for (int t = 0; t < lp.n_max_gaps; t++) {
            wave_sync();
            for (int j = lane; j < n; j += 64) {
                const uint32_t k = C.id[j];
                XF sacc{0.0, 0};
                for (uint32_t e = a.M.par_off[k]; e < a.M.par_off[k + 1]; e++) {
                    const int q = xl_find(C, a.M.par_node[e]);
                    if (q < 0) continue;
                    sacc = xf_add(sacc, xf_mul(XF{src[q], srce[q]}, trans[a.M.par_edge[e]] * lp.p_DD));
                }
                dst[j] = sacc.m;
                dste[j] = sacc.e;
                const XF dv = xf_add(XF{C.d[j], C.de[j]}, sacc);
                C.d[j] = dv.m;
                C.de[j] = dv.e;
            }
            double *tmp = src;
            src = dst;
            dst = tmp;
            int *tmpe = srce;
            srce = dste;
            dste = tmpe;
        }
        wave_sync();
        np = n;
    }
    // fe over the last column's list
    double lpv = -INFINITY;
    if (!bad && len > 0) {
        const XCol &L = cols[cur ^ 1];
        XF e{0.0, 0};
        for (int j = lane; j < np; j += 64)
            e = xf_add(e, xf_add(xf_add(XF{L.m[j], L.me[j]}, XF{L.i[j], L.ie[j]}), XF{L.d[j], L.de[j]}));
        for (int off = 32; off >= 1; off >>= 1) {
            XF o;
            o.m = __shfl_xor(e.m, off);
            o.e = __shfl_xor(e.e, off);
            e = xf_add(e, o);
        }
        lpv = xf_log(xf_mul(e, lp.p_end));
    }
    if (lane == 0) res[blockIdx.x] = bad ? NAN : lpv;
}

__global__ void __launch_bounds__(256) exp_kernel(const double *in, double *out, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const double v = in[i];
        out[i] = v == -INFINITY ? 0.0 : exp(v);
    }
}

void upload_reads(const phmm_reads *r) {
    if (r->on_device) return;
    r->d_bases.upload(r->bases.data(), r->bases.size());
    r->d_off.upload(r->off.data(), r->off.size() * sizeof(uint64_t));
    HIP_CHECK(hipStreamSynchronize(current_stream()));
    r->on_device = true;
}
void upload_mappings(const phmm_mappings *mp) {
    if (mp->on_device) return;
    mp->d_pos_off.upload(mp->pos_off.data(), mp->pos_off.size() * sizeof(uint64_t));
    mp->d_nodes.upload(mp->nodes.data(), std::max<size_t>(mp->nodes.size(), 1) * sizeof(uint32_t));
    HIP_CHECK(hipStreamSynchronize(current_stream()));
    mp->on_device = true;
}

namespace {

SparseModel sparse_model(const phmm_model *m) {
    const ModelDev &d = m->dev;
    SparseModel s{};
    s.N = (int)m->N;
    s.emis = d.emis.as<uint8_t>();
    s.init = d.init.as<double>();
    s.par_off = d.par_off.as<uint32_t>();
    s.par_node = d.par_node.as<uint32_t>();
    s.par_edge = d.par_edge.as<uint32_t>();
    s.chi_off = d.chi_off.as<uint32_t>();
    s.chi_node = d.chi_node.as<uint32_t>();
    s.chi_edge = d.chi_edge.as<uint32_t>();
    s.trans = d.trans_lin.as<double>();
    s.prec = d.prec.as<ParRec>();
    s.lp = m->lin;
    s.logib = d.logib.as<double>();
    return s;
}

struct EvTimer {
    hipEvent_t a = nullptr, b = nullptr;
    bool on;
    explicit EvTimer(bool on_) : on(on_) {
        if (on) {
            HIP_CHECK(hipEventCreate(&a));
            HIP_CHECK(hipEventCreate(&b));
            HIP_CHECK(hipEventRecord(a, current_stream()));
        }
    }
    ~EvTimer() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
    double stop() {
        if (!on) return 0.0;
        HIP_CHECK(hipEventRecord(b, current_stream()));
        HIP_CHECK(hipEventSynchronize(b));
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, a, b));
        return ms;
    }
};

// The workspace slots of this file (WorkSet::aux, phmm_internal.h), by name.  A slot keeps its size across calls; what
// it holds changes with the phase of a call, and a phase that takes a slot over starts behind a stream synchronisation
// that ended the one before:
//   WS_LISTS      hinted_run: the launch lists of the packed classes, then those of the wide classes (their cell
//                 counter behind them), then the list of each generic class, then the pairs | results of the exact pass
//   WS_CNC_MASKS  cnc_score: node (group) masks | read masks of a stateless call until they are read back, then (handle
//                 calls too) pairs | gathered values | gathered error bits
//   WS_CNC_LIST   cnc_score: the marks {candidate, node} until the masks are read back, then base vector | changes
//   WS_STAGING    the caller's ln probabilities or copy-number vectors (the totals behind them) on their way to
//                 WS_CAND_INIT / WS_CAND_TRANS
//   WS_OUT        written by the hinted kernels; a handle's lk_compose / lk_commit read it after cnc_score
//   WS_LK_MASKS   handle calls: as WS_CNC_MASKS' first phase, kept until lk_compose / lk_commit have run
//   WS_LK_COMPOSE lk_run_compose: candidates | totals | [C][R] values; a move's change list behind that
// mapping_flow.hip and sparse_dyn.hip use slots 13 and 14 as well, in calls that never overlap these.
enum WsSlot {
    WS_CAND_INIT = 7,    // [C][N] init of the candidates, linear
    WS_CAND_TRANS = 8,   // [C][E] trans
    WS_STAGING = 9,
    WS_LISTS = 10,
    WS_OUT = 11,         // [C][R] ln P planes
    WS_ERR = 12,         // [C][R] error bits
    WS_LK_MASKS = 13,
    WS_LK_COMPOSE = 14,
    WS_CNC_MASKS = 22,
    WS_CNC_LIST = 23,
};
inline DevBuf &ws(phmm_model *m, WsSlot k) { return m->wset().aux[k]; }

// ---- the scheduler of the score-only hinted forward (hinted_run, below the change form's kernels)
// What a call scores.  Two shapes: the grid reads x planes (pairs == nullptr: the full form), or a list of
// {read, plane} pairs, read-major (the touched pairs of the change form).  pair_off counts the pairs of a read in
// either shape; which shape it is matters in hinted_list, hinted_errors and hinted_results only.
struct HintedWork {
    uint32_t planes = 0;      // candidates the kernels index: n_cand of the grid, the D dirty slots of a pair list
    uint32_t call_cands = 0;  // candidates of the call, for the packed classes (the change form: its C, not D)
    const uint64_t *pair_off = nullptr;  // [R + 1] first pair of each read (the grid: r x planes)
    const uint2 *pairs = nullptr;        // host {read, plane}
    const uint2 *d_pairs = nullptr;      // the pairs on the device, and room for a value and an error word each
    double *d_res = nullptr;
    uint32_t *d_rerr = nullptr;
    const RecPool *pool = nullptr;  // forward records (forward_with_mapping): one-candidate kernels, no exact pass
    bool scatter_exact = false;     // the planes are read after the call (a handle): the exact pass writes them too
    double *vals = nullptr;         // out, host: [planes][R] of the grid, one value per pair of a list
};
// One class's reads as a launch: `n` blocks of `stride` words from word `at` of the uploaded lists, grid.y = y.
// stride 1: a read id per block, its candidates by blockIdx.y (the kernels' plain form); above 1: work units
// {read, stride - 1 planes}, 0xffffffff for an idle slot (their PAIRS form).
struct HintedList {
    size_t at;
    unsigned n, y, stride;
};

// init_c / trans_c: [planes][N], [planes][E] linear; the result planes are reserved here
HintedArgs hinted_args(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mp, uint32_t planes,
                       const double *init_c, const double *trans_c, const RecPool *pool) {
    DevBuf &d_out = ws(m, WS_OUT), &d_err = ws(m, WS_ERR);
    d_out.reserve((size_t)planes * reads->R * sizeof(double));
    d_err.reserve((size_t)planes * reads->R * sizeof(uint32_t));
    HintedArgs a{};
    a.M = sparse_model(m);
    a.init_c = init_c;
    a.trans_c = trans_c;
    a.E = m->E;
    a.bases = reads->d_bases.as<uint8_t>();
    a.read_off = reads->d_off.as<uint64_t>();
    a.map_pos_off = mp->d_pos_off.as<uint64_t>();
    a.map_nodes = mp->d_nodes.as<uint32_t>();
    a.R = reads->R;
    a.out_logp = d_out.as<double>();
    a.err = d_err.as<uint32_t>();
    if (pool) a.pool = *pool;
    return a;
}
void hinted_run(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mp, HintedArgs a, const HintedWork &w);

// packed class c (lists of at most 8 / 16 / 32 nodes), cpl candidates per lane
template <bool PAIRS> void launch_hinted_packed(int c, int cpl, const HintedArgs &a, dim3 grid, uint32_t n_cand) {
    hipStream_t s = current_stream();
    if (cpl >= 2) {
        if (c == 0) hipLaunchKernelGGL((hinted_packed_kernel<8, 2, PAIRS>), grid, dim3(64), 0, s, a, n_cand);
        else if (c == 1) hipLaunchKernelGGL((hinted_packed_kernel<16, 2, PAIRS>), grid, dim3(64), 0, s, a, n_cand);
        else hipLaunchKernelGGL((hinted_packed_kernel<32, 2, PAIRS>), grid, dim3(64), 0, s, a, n_cand);
    } else {
        if (c == 0) hipLaunchKernelGGL((hinted_packed_kernel<8, 1, PAIRS>), grid, dim3(64), 0, s, a, n_cand);
        else if (c == 1) hipLaunchKernelGGL((hinted_packed_kernel<16, 1, PAIRS>), grid, dim3(64), 0, s, a, n_cand);
        else hipLaunchKernelGGL((hinted_packed_kernel<32, 1, PAIRS>), grid, dim3(64), 0, s, a, n_cand);
    }
}
// generic class c (lists of at most 64 / 128 / 400 nodes, 2 / 4 / 8 in-list parents per node), one wave per read and
// candidate; lean: class 0 on graphs of degree <= ADJ_DEG, which also takes {read, plane} units
void launch_hinted_generic(int c, bool lean, const HintedArgs &a, const HintedList &L) {
    hipStream_t s = current_stream();
    const dim3 grid(L.n, L.y);
    if (lean && L.stride > 1) hipLaunchKernelGGL(hinted_lean_kernel<true>, grid, dim3(64), 0, s, a);
    else if (lean) hipLaunchKernelGGL(hinted_lean_kernel<false>, grid, dim3(64), 0, s, a);
    else if (c == 0) hipLaunchKernelGGL((hinted_score_kernel<64, 2>), grid, dim3(64), 0, s, a);
    else if (c == 1) hipLaunchKernelGGL((hinted_score_kernel<128, 4>), grid, dim3(64), 0, s, a);
    else hipLaunchKernelGGL((hinted_score_kernel<400, 8>), grid, dim3(64), 0, s, a);
}

// hinted_wide_kernel: block class wc (0: lists of 65-128 nodes on 128 threads, 1: 129-400 on 448), cpb candidates per
// block.  Which block shape or cpb ran a candidate does not show in its bits (hinted_wide_kernel.h).
static constexpr uint32_t HW_MAX_LIST = 400;
inline int hinted_wide_class(uint32_t mx) { return mx <= 128 ? 0 : 1; }
// Candidates per block.  A guess, not a measurement: sharing a position's topology work among candidates is taken to
// pay once the launch has 2 (4) times the pairs that 256 CUs hold as blocks of one candidate -- by registers 10 blocks
// of 128 threads, 2 of 448 per CU (more candidates per block lower that to 6 / 4 resp. 2) --
// and below that a block per pair keeps every read's chain of positions as short as it can be.
inline int hinted_wide_cpb(int wc, uint64_t n_reads, uint64_t n_pairs) {
    const uint64_t resident = wc == 0 ? 2560 : 512;
    const uint64_t per_read = n_reads ? n_pairs / n_reads : 0;
    int cpb = 1;
    if (per_read >= 2 && n_pairs >= 2 * resident) cpb = 2;
    if (per_read >= 4 && n_pairs >= 4 * resident) cpb = 4;
    if (knobs().wide_hinted_cpb > 0) cpb = knobs().wide_hinted_cpb;  // (tests: every shape gives the same bits)
    return wc == 0 ? (cpb >= 4 ? 4 : (cpb >= 2 ? 2 : 1)) : (cpb >= 2 ? 2 : 1);
}
template <bool PAIRS> void launch_hinted_wide(int wc, int cpb, const HintedArgs &a, dim3 grid, uint32_t n_cand) {
    hipStream_t s = current_stream();
    if (a.pool.base) {
        // stored columns (forward_with_mapping): one candidate, one block per read, a record per position
        if constexpr (PAIRS) PHMM_THROW(PHMM_EINTERNAL, "hinted wide class: stored columns on work units");
        else if (wc == 0) hipLaunchKernelGGL((hinted_wide_kernel<128, 1, false, true>), grid, dim3(128), 0, s, a, n_cand);
        else hipLaunchKernelGGL((hinted_wide_kernel<448, 1, false, true>), grid, dim3(448), 0, s, a, n_cand);
    } else if (wc == 0) {
        if (cpb >= 4) hipLaunchKernelGGL((hinted_wide_kernel<128, 4, PAIRS>), grid, dim3(128), 0, s, a, n_cand);
        else if (cpb == 2) hipLaunchKernelGGL((hinted_wide_kernel<128, 2, PAIRS>), grid, dim3(128), 0, s, a, n_cand);
        else hipLaunchKernelGGL((hinted_wide_kernel<128, 1, PAIRS>), grid, dim3(128), 0, s, a, n_cand);
    } else {
        if (cpb >= 2) hipLaunchKernelGGL((hinted_wide_kernel<448, 2, PAIRS>), grid, dim3(448), 0, s, a, n_cand);
        else hipLaunchKernelGGL((hinted_wide_kernel<448, 1, PAIRS>), grid, dim3(448), 0, s, a, n_cand);
    }
}
// The cells of a wide launch for the call statistics (list entries of the read x its candidates), added to *out on the
// device: the position offsets of device-resident mappings are not on the host.  Units of `stride` words: {read} with
// per_unit candidates each (stride 1), or {read, stride - 1 candidate slots} with 0xffffffff for an idle slot.
__global__ void __launch_bounds__(256) hinted_wide_cells(const uint32_t *units, uint32_t n_units, uint32_t stride,
                                                         uint32_t per_unit, const uint64_t *read_off,
                                                         const uint64_t *map_pos_off, unsigned long long *out) {
    const uint32_t u = blockIdx.x * 256 + threadIdx.x;
    unsigned long long s = 0;
    if (u < n_units) {
        const uint32_t *w = units + (size_t)u * stride;
        uint32_t k = per_unit;
        if (stride > 1) {
            k = 0;
            for (uint32_t j = 1; j < stride; j++) k += w[j] != 0xffffffffu;
        }
        s = (unsigned long long)(map_pos_off[read_off[w[0] + 1]] - map_pos_off[read_off[w[0]]]) * k;
    }
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(out, s);
}
inline void launch_hinted_wide_cells(const HintedArgs &a, uint32_t n_units, uint32_t stride, uint32_t per_unit,
                                     unsigned long long *d_cells) {
    hipLaunchKernelGGL(hinted_wide_cells, dim3((n_units + 255) / 256), dim3(256), 0, current_stream(), a.read_ids, n_units,
                       stride, per_unit, a.read_off, a.map_pos_off, d_cells);
}

}  // namespace

// Candidate (init, trans) vectors straight from copy-number vectors, in the linear domain
// (SeqGraph::to_phmm_node / to_phmm_edge without edge copy numbers, seq_graph.rs:160-209, with
// total_emittable_copy_num / total_emittable_child_copy_nums, seq_graph.rs:110-135):
//   init[v]        = emittable(v) ? max(cn[v], min) / sum_{emittable u} max(cn[u], min) : 0
//   trans[v -> w]  = emittable(w) and T_v > 0 ? max(cn[w], min) / T_v : 0,
//   T_v            = sum over the emittable children u of v of max(cn[u], min)
// Copy numbers are integers: the sums are exact and order-independent.
__global__ void __launch_bounds__(256) cn_totals(const uint32_t *cn, const uint8_t *emis, uint32_t N, uint32_t min_cn,
                                                 unsigned long long *tot) {
    const uint32_t c = blockIdx.y;
    unsigned long long s = 0;
    for (uint32_t v = blockIdx.x * 256 + threadIdx.x; v < N; v += gridDim.x * 256)
        if (emis[v] != (uint8_t)'n') s += max(cn[(size_t)c * N + v], min_cn);
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(&tot[c], s);
}
__global__ void __launch_bounds__(256) cn_probs(const uint32_t *cn, const uint8_t *emis, const uint32_t *chi_off,
                                                const uint32_t *chi_node, const uint32_t *chi_edge, uint32_t N, uint32_t E,
                                                uint32_t min_cn, const unsigned long long *tot, double *init, double *trans) {
    const uint32_t c = blockIdx.y;
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v >= N) return;
    const uint32_t *cc = cn + (size_t)c * N;
    const unsigned long long total = tot[c];
    init[(size_t)c * N + v] = (emis[v] != (uint8_t)'n' && total > 0) ? (double)max(cc[v], min_cn) / (double)total : 0.0;
    unsigned long long tv = 0;
    for (uint32_t a = chi_off[v]; a < chi_off[v + 1]; a++) {
        const uint32_t u = chi_node[a];
        if (emis[u] != (uint8_t)'n') tv += max(cc[u], min_cn);
    }
    for (uint32_t a = chi_off[v]; a < chi_off[v + 1]; a++) {
        const uint32_t u = chi_node[a];
        const uint32_t k = max(cc[u], min_cn);
        trans[(size_t)c * E + chi_edge[a]] = (emis[u] != (uint8_t)'n' && tv > 0 && k > 0) ? (double)k / (double)tv : 0.0;
    }
}

namespace {
// init / trans of the n_cand copy-number vectors d_cn [n_cand][N] into WS_CAND_INIT / WS_CAND_TRANS; d_tot: n_cand
// zeroed words
void copy_num_probs(phmm_model *m, const uint32_t *d_cn, uint32_t n_cand, uint32_t min_cn, unsigned long long *d_tot) {
    hipStream_t s = current_stream();
    const uint32_t N = m->N, E = m->E;
    DevBuf &cand_init = ws(m, WS_CAND_INIT), &cand_trans = ws(m, WS_CAND_TRANS);
    cand_init.reserve((size_t)n_cand * N * sizeof(double));
    cand_trans.reserve(std::max<size_t>((size_t)n_cand * E, 1) * sizeof(double));
    const unsigned nb = (unsigned)((N + 255) / 256);
    hipLaunchKernelGGL(cn_totals, dim3(std::min(nb, 256u), n_cand), dim3(256), 0, s, d_cn, m->dev.emis.as<uint8_t>(), N, min_cn,
                       d_tot);
    hipLaunchKernelGGL(cn_probs, dim3(nb, n_cand), dim3(256), 0, s, d_cn, m->dev.emis.as<uint8_t>(),
                       m->dev.chi_off.as<uint32_t>(), m->dev.chi_node.as<uint32_t>(), m->dev.chi_edge.as<uint32_t>(), N, E,
                       min_cn, (const unsigned long long *)d_tot, cand_init.as<double>(), cand_trans.as<double>());
    HIP_CHECK(hipGetLastError());
}
}  // namespace

void full_prob_reads_hinted(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mp, uint32_t n_cand,
                            const double *init_logp, const double *trans_logp, double *out_logp,
                            double *out_total, const RecPool *pool, const uint32_t *copy_nums, uint32_t min_copy_num) {
    hipStream_t s = current_stream();
    CallStats &st = stats();
    st = CallStats();
    const uint64_t R = reads->R;
    const uint32_t N = m->N, E = m->E;
    if (m->dev.max_degree > 8)
        PHMM_THROW(PHMM_EINVAL, "sparse path supports node degree <= 8 (MultiDbg MAX_DEGREE is 5)");
    upload_reads(reads);
    upload_mappings(mp);
    ensure_logib(m, reads->max_len + 1);

    // candidate probabilities in the linear domain: [C][N], [C][E]
    DevBuf &cand_init = ws(m, WS_CAND_INIT), &cand_trans = ws(m, WS_CAND_TRANS), &staging = ws(m, WS_STAGING);
    const double *d_init = m->dev.init.as<double>();
    const double *d_trans = m->dev.trans_lin.as<double>();
    if (init_logp) {
        const size_t ni = (size_t)n_cand * N, ne = (size_t)n_cand * E;
        staging.reserve(std::max(ni, ne) * sizeof(double));
        cand_init.reserve(ni * sizeof(double));
        cand_trans.reserve(std::max<size_t>(ne, 1) * sizeof(double));
        HIP_CHECK(hipMemcpyAsync(staging.p, init_logp, ni * sizeof(double), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(exp_kernel, dim3((unsigned)((ni + 255) / 256)), dim3(256), 0, s, staging.as<double>(),
                           cand_init.as<double>(), ni);
        if (ne) {
            HIP_CHECK(hipStreamSynchronize(s));
            HIP_CHECK(hipMemcpyAsync(staging.p, trans_logp, ne * sizeof(double), hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(exp_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, s, staging.as<double>(),
                               cand_trans.as<double>(), ne);
        }
        HIP_CHECK(hipStreamSynchronize(s));
        d_init = cand_init.as<double>();
        d_trans = cand_trans.as<double>();
    } else if (copy_nums) {
        const size_t ni = (size_t)n_cand * N;
        staging.reserve(ni * sizeof(uint32_t) + 256 + n_cand * sizeof(unsigned long long));
        uint32_t *d_cn = staging.as<uint32_t>();
        unsigned long long *d_tot = (unsigned long long *)(staging.as<char>() + (ni * sizeof(uint32_t) + 255) / 256 * 256);
        HIP_CHECK(hipMemcpyAsync(d_cn, copy_nums, ni * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemsetAsync(d_tot, 0, n_cand * sizeof(unsigned long long), s));
        copy_num_probs(m, d_cn, n_cand, min_copy_num, d_tot);
        HIP_CHECK(hipStreamSynchronize(s));  // the caller's copy_nums may go away
        d_init = cand_init.as<double>();
        d_trans = cand_trans.as<double>();
    }

    // the grid reads x candidates through the scheduler
    std::vector<double> h_out((size_t)n_cand * R);
    std::vector<uint64_t> pair_off(R + 1);
    for (uint64_t r = 0; r <= R; r++) pair_off[r] = r * n_cand;
    HintedWork w;
    w.planes = w.call_cands = n_cand;
    w.pair_off = pair_off.data();
    w.pool = pool;
    w.vals = h_out.data();
    const HintedArgs a = hinted_args(m, reads, mp, n_cand, d_init, d_trans, pool);
    EvTimer tm(timing_enabled());
    hinted_run(m, reads, mp, a, w);
    if (pool) {
        // generate_mappings WITH lists (forward + backward over the lists): the backward pass needs the forward columns
        // of the scaled kernels, which a read that every list node cuts (a k-mer at probability 0 on its path) does not
        // have.  The reference calls this on to_non_zero_phmm (multi_dbg/posterior.rs:609-618), where no transition
        // is 0; a model that cuts a read is refused here instead of returning -inf / NaN posteriors.
        for (uint64_t r = 0; r < R; r++)
            if (h_out[r] == -INFINITY && reads->off[r + 1] > reads->off[r])
                PHMM_THROW(PHMM_EINVAL, "generate_mappings with mappings: read " + std::to_string(r) +
                                            " has probability 0 on its lists under this model (a zero-copy k-mer cuts it); "
                                            "use the non-zero PHMM (to_non_zero_phmm) for mapping, as the reference does");
    }
    st.ms[2] += tm.stop();
    st.cells[2] = mp->total_entries * n_cand;

    std::vector<double> tot(n_cand, 0.0);
    for (uint32_t k = 0; k < n_cand; k++)
        for (uint64_t r = 0; r < R; r++) tot[k] += h_out[(size_t)k * R + r];  // rayon .product(): sum of logs
    put_doubles(out_logp, h_out.data(), h_out.size());
    put_doubles(out_total, tot.data(), n_cand);
}

// ---------------------------------------------------------------- candidates as changes to a base vector
// phmm_full_prob_reads_copy_num_changes: the loop of sample_posterior_once (posterior.rs:483-515) rescoring only the
// reads a candidate touches.  With e(v) = max(cn(v), min_copy_num), T = sum of e over the emittable nodes, D_c the nodes
// whose e differs from the base and A_c = D_c + parents(D_c): a read none of whose listed nodes is in A_c sees every
// listed init scaled by T_base / T_c and every trans it uses unchanged (forward_with_mapping reads only those, and
// every path takes exactly one init term), so ln P_c = ln P_base + ln(T_base / T_c).  DESIGN.md section 6.

// bit c % 64 of word c / 64 in the mask of v and of every parent of v, per effective change {c, v}
__global__ void __launch_bounds__(256) cnc_mark(const uint2 *chg, uint32_t n_chg, const uint32_t *par_off,
                                                const uint32_t *par_node, uint32_t N, unsigned long long *node_mask) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_chg) return;
    const uint32_t c = chg[j].x, v = chg[j].y;
    const unsigned long long bit = 1ull << (c & 63);
    unsigned long long *w = node_mask + (size_t)(c >> 6) * N;
    atomicOr(&w[v], bit);
    for (uint32_t q = par_off[v]; q < par_off[v + 1]; q++) atomicOr(&w[par_node[q]], bit);
}
// one wave per read: the OR of the mask words of every entry of its lists; word blockIdx.y
__global__ void __launch_bounds__(256) cnc_read_mask(const uint64_t *read_off, uint64_t R, const uint64_t *map_pos_off,
                                                     const uint32_t *map_nodes, uint32_t N,
                                                     const unsigned long long *node_mask, unsigned long long *read_mask) {
    const uint64_t r = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const unsigned long long *w = node_mask + (size_t)blockIdx.y * N;
    const uint64_t e0 = map_pos_off[read_off[r]], e1 = map_pos_off[read_off[r + 1]];
    unsigned long long acc = 0;
    for (uint64_t e = e0 + (threadIdx.x & 63); e < e1; e += 64) acc |= w[map_nodes[e]];
    for (int off = 32; off >= 1; off >>= 1) acc |= __shfl_xor(acc, off);
    if ((threadIdx.x & 63) == 0) read_mask[(size_t)blockIdx.y * R + r] = acc;
}
// Group flavours (phmm_likelihood_set_groups): the mask table of one word has S = G + P entries, a word per group and
// a word per distinct boundary parent (a parent of a node of some group that is not in that group), instead of N.
// bit c % 64 of word c / 64 in the entry of g and of each boundary parent of g, per effective change {c, g}
__global__ void __launch_bounds__(256) cng_mark(const uint2 *chg, uint32_t n_chg, const uint32_t *bp_off,
                                                const uint32_t *bp_slot, uint32_t G, uint32_t S,
                                                unsigned long long *slot_mask) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_chg) return;
    const uint32_t c = chg[j].x, g = chg[j].y;
    const unsigned long long bit = 1ull << (c & 63);
    unsigned long long *w = slot_mask + (size_t)(c >> 6) * S;
    atomicOr(&w[g], bit);
    for (uint32_t q = bp_off[g]; q < bp_off[g + 1]; q++) atomicOr(&w[G + bp_slot[q]], bit);
}
// cnc_read_mask over that table: per list entry v the word of its group and its own word as a boundary parent
// (node_slot[v] = {group, boundary-parent slot}, 0xffffffff for none) -- A_c = D_c + parents(D_c), as the node form
__global__ void __launch_bounds__(256) cng_read_mask(const uint64_t *read_off, uint64_t R, const uint64_t *map_pos_off,
                                                     const uint32_t *map_nodes, const uint2 *node_slot, uint32_t G,
                                                     uint32_t S, const unsigned long long *slot_mask,
                                                     unsigned long long *read_mask) {
    const uint64_t r = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const unsigned long long *w = slot_mask + (size_t)blockIdx.y * S;
    const uint64_t e0 = map_pos_off[read_off[r]], e1 = map_pos_off[read_off[r + 1]];
    unsigned long long acc = 0;
    for (uint64_t e = e0 + (threadIdx.x & 63); e < e1; e += 64) {
        const uint2 sl = node_slot[map_nodes[e]];
        if (sl.x != 0xffffffffu) acc |= w[sl.x];
        if (sl.y != 0xffffffffu) acc |= w[G + sl.y];
    }
    for (int off = 32; off >= 1; off >>= 1) acc |= __shfl_xor(acc, off);
    if ((threadIdx.x & 63) == 0) read_mask[(size_t)blockIdx.y * R + r] = acc;
}
// copy-number vectors of the D candidates with a dirty read: the base, then their changes {slot, node, cn}
__global__ void __launch_bounds__(256) cnc_expand(const uint32_t *base, uint32_t N, uint32_t *cn) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v < N) cn[(size_t)blockIdx.y * N + v] = base[v];
}
__global__ void __launch_bounds__(256) cnc_apply(const uint3 *chg, uint32_t n_chg, uint32_t N, uint32_t *cn) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j < n_chg) cn[(size_t)chg[j].x * N + chg[j].y] = chg[j].z;
}
// changes {slot, group, cn}: a block per change writes cn over the group's nodes
__global__ void __launch_bounds__(256) cng_apply(const uint3 *chg, const uint64_t *g_off, const uint32_t *g_nodes,
                                                 uint32_t N, uint32_t *cn) {
    const uint3 t = chg[blockIdx.x];
    uint32_t *o = cn + (size_t)t.x * N;
    for (uint64_t i = g_off[t.y] + threadIdx.x; i < g_off[t.y + 1]; i += 256) o[g_nodes[i]] = t.z;
}
// results of the pairs {read, slot} out of the [D][R] planes the scoring kernels write
__global__ void __launch_bounds__(256) cnc_gather(const uint2 *pairs, size_t n, uint64_t R, const double *out,
                                                  const uint32_t *err, double *res, uint32_t *res_err) {
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    const size_t k = (size_t)pairs[q].y * R + pairs[q].x;
    res[q] = out[k];
    res_err[q] = err[k];
}

// results of the exact pass over the pairs {slot, read} back into the [D][R] planes (NaN: the plane's value stands)
__global__ void __launch_bounds__(256) cnc_scatter(const uint2 *pairs, const double *res, size_t n, uint64_t R,
                                                   double *out) {
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    const double v = res[q];
    if (v == v) out[(size_t)pairs[q].x * R + pairs[q].y] = v;
}

namespace {

// ---------------------------------------------------------------- the scheduler of the score-only hinted forward
// Which read goes to which kernel, what becomes of a read a kernel flags, and which pairs take the exact pass, for the
// full form's grid and the change form's pair list alike (HintedWork).

// Generic class of a longest list of mx nodes
inline int hinted_generic_class(uint32_t mx) { return mx <= 64 ? 0 : (mx <= 128 ? 1 : 2); }

// The reads `rds` of one class as a launch, appended to `words`.  The grid, and the generic kernels in either shape
// (whole_reads), take the read ids x ceil(planes / per_unit) in y; a pair list becomes work units of per_unit planes.
// The generic kernels run over a class's reads x every plane and only the pairs are read back: a pair-list instantiation
// of hinted_score_kernel would change the register allocation of the shared fwd_list_step in the reads x candidates
// one, and a launch per candidate serialises long reads.
HintedList hinted_list(const HintedWork &w, const std::vector<uint32_t> &rds, unsigned per_unit, bool whole_reads,
                       std::vector<uint32_t> &words) {
    HintedList L{words.size(), 0, 1, 1};
    if (!w.pairs || whole_reads) {
        words.insert(words.end(), rds.begin(), rds.end());
        L.n = (unsigned)rds.size();
        L.y = (w.planes + per_unit - 1) / per_unit;
        return L;
    }
    L.stride = 1 + per_unit;
    for (uint32_t r : rds)
        for (uint64_t q = w.pair_off[r]; q < w.pair_off[r + 1]; q += per_unit) {
            words.push_back(r);
            for (unsigned k = 0; k < per_unit; k++)
                words.push_back(q + k < w.pair_off[r + 1] ? w.pairs[q + k].y : 0xffffffffu);
        }
    L.n = (unsigned)((words.size() - L.at) / L.stride);
    return L;
}

void launch_cnc_gather(const HintedArgs &a, const HintedWork &w) {
    const size_t n = w.pair_off[a.R];
    hipLaunchKernelGGL(cnc_gather, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, current_stream(), w.d_pairs, n, a.R,
                       (const double *)a.out_logp, (const uint32_t *)a.err, w.d_res, w.d_rerr);
    HIP_CHECK(hipGetLastError());
}

// Once the launches before it have finished: the error bits of every read of the n_lists class lists, OR-ed over the
// read's candidates, in list order
void hinted_errors(const HintedArgs &a, const HintedWork &w, const std::vector<uint32_t> *lists, int n_lists,
                   std::vector<uint32_t> &h_err, std::vector<uint32_t> &read_err) {
    hipStream_t s = current_stream();
    const uint64_t R = a.R;
    read_err.clear();
    if (!w.pairs) {
        h_err.resize((size_t)w.planes * R);
        HIP_CHECK(hipMemcpyAsync(h_err.data(), a.err, h_err.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        for (int c = 0; c < n_lists; c++)
            for (uint32_t rd : lists[c]) {
                uint32_t e = 0;
                for (uint32_t k = 0; k < w.planes; k++) e |= h_err[(size_t)k * R + rd];
                read_err.push_back(e);
            }
        return;
    }
    h_err.resize(w.pair_off[R]);
    launch_cnc_gather(a, w);
    HIP_CHECK(hipMemcpyAsync(h_err.data(), w.d_rerr, h_err.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    for (int c = 0; c < n_lists; c++)
        for (uint32_t rd : lists[c]) {
            uint32_t e = 0;
            for (uint64_t q = w.pair_off[rd]; q < w.pair_off[rd + 1]; q++) e |= h_err[q];
            read_err.push_back(e);
        }
}

// What becomes of a read whose error bits are e: nothing (-1), the generic class that takes it next, or a throw.
// stage 0: a packed class flagged it, 1: a wide class, 2: the generic class c.
int hinted_route(uint32_t e, int stage, int c, uint32_t max_list) {
    if (!e) return -1;
    if (e & SP_ERR_POOL) PHMM_THROW(PHMM_EINTERNAL, "forward record pool exhausted");
    if (e & SP_ERR_DUPLICATE) PHMM_THROW(PHMM_EINVAL, "duplicate node in a mapping list");
    if (stage == 0) return 0;  // (cannot happen with read_max_list right: the one-candidate kernels take it)
    if (stage == 1) return hinted_generic_class(max_list);  // the generic kernel reports what it finds
    // reads whose in-list fan-in exceeded this class's link budget are promoted
    if ((e & (SP_ERR_LINKS | SP_ERR_CAPACITY)) && c < 2) return c + 1;
    PHMM_THROW(PHMM_ECAPACITY, "mapping list needs more than 400 slots / 8 in-list parents");
}

// A pair that came back -inf, and where its value lives in w.vals
struct HintedCut {
    uint32_t plane, read;
    size_t at;
};
// The values of the call into w.vals; the -inf pairs of non-empty reads in `cut`, in the order of w.vals
void hinted_results(const HintedArgs &a, const HintedWork &w, const phmm_reads *reads, std::vector<HintedCut> &cut) {
    hipStream_t s = current_stream();
    const uint64_t R = a.R;
    if (!w.pairs) {
        HIP_CHECK(hipMemcpyAsync(w.vals, a.out_logp, (size_t)w.planes * R * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        for (uint32_t k = 0; k < w.planes; k++)
            for (uint64_t r = 0; r < R; r++)
                if (w.vals[(size_t)k * R + r] == -INFINITY && reads->off[r + 1] > reads->off[r])
                    cut.push_back(HintedCut{k, (uint32_t)r, (size_t)k * R + r});
        return;
    }
    const size_t n = w.pair_off[R];  // (pairs of non-empty reads only)
    launch_cnc_gather(a, w);
    HIP_CHECK(hipMemcpyAsync(w.vals, w.d_res, n * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    for (size_t q = 0; q < n; q++)
        if (w.vals[q] == -INFINITY) cut.push_back(HintedCut{w.pairs[q].y, w.pairs[q].x, q});
}

// (candidate, read) pairs that came back -inf: the reference's InsBegin chain may still carry them (see
// hinted_exact_kernel) -- recomputed in its own arithmetic
void hinted_exact_pass(phmm_model *m, const phmm_mappings *mp, const HintedArgs &a, const HintedWork &w,
                       std::vector<HintedCut> &cut) {
    if (cut.empty()) return;
    hipStream_t s = current_stream();
    // short lists first (the small kernel), the rest behind them
    const size_t n = cut.size();
    const size_t n_small = (size_t)(std::stable_partition(cut.begin(), cut.end(), [&](const HintedCut &q) {
                                        return mp->read_max_list[q.read] <= 64;
                                    }) - cut.begin());
    std::vector<uint2> xs(n);  // {plane, read}
    for (size_t i = 0; i < n; i++) xs[i] = make_uint2(cut[i].plane, cut[i].read);
    DevBuf &buf = ws(m, WS_LISTS);  // (the launch lists are spent)
    const size_t res_at = (n * sizeof(uint2) + 255) / 256 * 256;
    buf.reserve(res_at + n * sizeof(double));
    uint2 *dp = buf.as<uint2>();
    double *dres = (double *)(buf.as<char>() + res_at);
    HIP_CHECK(hipMemcpyAsync(dp, xs.data(), n * sizeof(uint2), hipMemcpyHostToDevice, s));
    if (n_small)
        hipLaunchKernelGGL((hinted_exact_kernel<64, 256>), dim3((unsigned)n_small), dim3(64), 0, s, a, (const uint2 *)dp, dres);
    if (n_small < n)
        hipLaunchKernelGGL((hinted_exact_kernel<PHMM_MAX_ACTIVE_NODES, 1024>), dim3((unsigned)(n - n_small)), dim3(64), 0, s,
                           a, (const uint2 *)(dp + n_small), dres + n_small);
    if (w.scatter_exact)
        hipLaunchKernelGGL(cnc_scatter, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const uint2 *)dp,
                           (const double *)dres, n, a.R, a.out_logp);
    HIP_CHECK(hipGetLastError());
    std::vector<double> hres(n);
    HIP_CHECK(hipMemcpyAsync(hres.data(), dres, n * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    for (size_t i = 0; i < n; i++)
        if (hres[i] == hres[i]) w.vals[cut[i].at] = hres[i];
    stats().launches[2]++;
}

void hinted_run(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mp, HintedArgs a, const HintedWork &w) {
    hipStream_t s = current_stream();
    CallStats &st = stats();
    const uint64_t R = reads->R;
    DevBuf &d_lists = ws(m, WS_LISTS);
    // capacity classes by the longest node list of each read.  Candidate batches: reads with short lists go to the
    // packed kernels (several candidates per wave) first.
    const bool lean_ok = m->dev.max_degree <= (uint32_t)ADJ_DEG && !knobs().no_lean;
    const bool packed_ok = w.call_cands >= 2 && !w.pool && lean_ok && !knobs().no_packed;
    // lists of 65-400 nodes: one block per read (hinted_wide_kernel.h).  By the read's lists, the model and the knobs
    // only -- never by the candidate count: a batch stays bit-equal to one-candidate calls.  The class is opt-in
    // (PHMM_WIDE_HINTED): speed is its only purpose, and the timings so far do not make it the
    // default.  A call that stores the columns (w.pool: forward_with_mapping) takes the record-storing flavour; a read
    // the class flags is redone by the generic class, whose records replace the block's (pool.off[] points at the later
    // record, the earlier bytes stay unused)
    const bool wide_ok = lean_ok && knobs().wide_hinted;
    std::vector<uint32_t> cls[3], pcls[3], wcls[2];
    for (uint64_t r = 0; r < R; r++) {
        if (w.pair_off[r + 1] == w.pair_off[r]) continue;
        const uint32_t mx = mp->read_max_list[r];
        if (packed_ok && mx <= 32) pcls[mx <= 8 ? 0 : (mx <= 16 ? 1 : 2)].push_back((uint32_t)r);
        else if (wide_ok && mx > 64 && mx <= HW_MAX_LIST) wcls[hinted_wide_class(mx)].push_back((uint32_t)r);
        else cls[hinted_generic_class(mx)].push_back((uint32_t)r);
    }
    auto class_pairs = [&](const std::vector<uint32_t> &rds) {
        uint64_t np = 0;
        for (uint32_t r : rds) np += w.pair_off[r + 1] - w.pair_off[r];
        return np;
    };
    std::vector<uint32_t> words, h_err, read_err;
    HintedList L[3];

    // packed classes: candidates per wave = (64 / WG) x CPL; two per lane once a class has that many pairs per read
    // on average.  The three classes behind one upload.
    int cpl[3];
    for (int c = 0; c < 3; c++) {
        const int G = c == 0 ? 8 : (c == 1 ? 4 : 2);
        const int cpl_env = knobs().packed_cpl;
        cpl[c] = (cpl_env > 0 ? cpl_env >= 2 : class_pairs(pcls[c]) >= (uint64_t)(2 * G) * pcls[c].size()) ? 2 : 1;
        L[c] = hinted_list(w, pcls[c], (unsigned)(G * cpl[c]), false, words);
    }
    if (!words.empty()) {
        d_lists.reserve(words.size() * sizeof(uint32_t));
        HIP_CHECK(hipMemcpyAsync(d_lists.p, words.data(), words.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        for (int c = 0; c < 3; c++) {
            if (!L[c].n) continue;
            a.read_ids = d_lists.as<uint32_t>() + L[c].at;
            if (L[c].stride > 1) launch_hinted_packed<true>(c, cpl[c], a, dim3(L[c].n, L[c].y), w.planes);
            else launch_hinted_packed<false>(c, cpl[c], a, dim3(L[c].n, L[c].y), w.planes);
            HIP_CHECK(hipGetLastError());
            st.launches[2]++;
        }
        hinted_errors(a, w, pcls, 3, h_err, read_err);
        size_t i = 0;
        for (int c = 0; c < 3; c++)
            for (uint32_t rd : pcls[c])
                if (hinted_route(read_err[i++], 0, c, 0) >= 0) cls[0].push_back(rd);
    }
    trace("hinted: packed classes");
    // wide lists (65-400 nodes): the two classes behind one upload, the cell counter of the call statistics behind them
    if (!wcls[0].empty() || !wcls[1].empty()) {
        EvTimer tw(timing_enabled());
        words.clear();
        int cpb[2];
        for (int wc = 0; wc < 2; wc++) {
            // (a stored-column call is one candidate: one per block whatever the knob says)
            cpb[wc] = w.pool ? 1 : hinted_wide_cpb(wc, wcls[wc].size(), class_pairs(wcls[wc]));
            L[wc] = hinted_list(w, wcls[wc], (unsigned)cpb[wc], false, words);
        }
        const size_t cells_at = (words.size() * sizeof(uint32_t) + 7) / 8 * 8;
        d_lists.reserve(cells_at + sizeof(unsigned long long));
        unsigned long long *d_cells = (unsigned long long *)(d_lists.as<char>() + cells_at), h_cells = 0;
        HIP_CHECK(hipMemcpyAsync(d_lists.p, words.data(), words.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemsetAsync(d_cells, 0, sizeof(unsigned long long), s));
        for (int wc = 0; wc < 2; wc++) {
            if (!L[wc].n) continue;
            a.read_ids = d_lists.as<uint32_t>() + L[wc].at;
            if (L[wc].stride > 1) launch_hinted_wide<true>(wc, cpb[wc], a, dim3(L[wc].n, L[wc].y), w.planes);
            else launch_hinted_wide<false>(wc, cpb[wc], a, dim3(L[wc].n, L[wc].y), w.planes);
            launch_hinted_wide_cells(a, L[wc].n, L[wc].stride, w.planes, d_cells);
            HIP_CHECK(hipGetLastError());
            st.launches[2]++;
            st.launches[4]++;
        }
        HIP_CHECK(hipMemcpyAsync(&h_cells, d_cells, sizeof(h_cells), hipMemcpyDeviceToHost, s));
        hinted_errors(a, w, wcls, 2, h_err, read_err);
        st.cells[4] += h_cells;
        size_t i = 0;
        for (int wc = 0; wc < 2; wc++)
            for (uint32_t rd : wcls[wc]) {
                const int to = hinted_route(read_err[i++], 1, wc, mp->read_max_list[rd]);
                if (to >= 0) cls[to].push_back(rd);
            }
        st.ms[4] += tw.stop();
    }
    trace("hinted: wide classes");
    // one-candidate classes, a launch and a read-back each: a read any of whose candidates overflows a class is
    // appended to the next one.  Class 0 runs the lean kernel where the graph allows it; the generic kernels take what
    // the lean and the wide class do not (degree above ADJ_DEG, PHMM_NO_LEAN set, lists over 64 nodes while the wide
    // class is not switched on, or a read one of them flagged).
    for (int c = 0; c < 3; c++) {
        if (cls[c].empty()) continue;
        const bool lean = c == 0 && lean_ok;
        words.clear();
        const HintedList Lc = hinted_list(w, cls[c], 1, !lean, words);
        d_lists.reserve(words.size() * sizeof(uint32_t));
        HIP_CHECK(hipMemcpyAsync(d_lists.p, words.data(), words.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        a.read_ids = d_lists.as<uint32_t>();
        launch_hinted_generic(c, lean, a, Lc);
        HIP_CHECK(hipGetLastError());
        st.launches[2]++;
        hinted_errors(a, w, &cls[c], 1, h_err, read_err);
        for (size_t i = 0; i < read_err.size(); i++) {
            const int to = hinted_route(read_err[i], 2, c, 0);
            if (to >= 0) cls[to].push_back(cls[c][i]);
        }
    }
    std::vector<HintedCut> cut;
    hinted_results(a, w, reads, cut);
    trace("hinted: one-candidate classes");
    if (!w.pool && !knobs().no_exact_hinted) hinted_exact_pass(m, mp, a, w, cut);
    trace("hinted: exact pass");
}

// One batch of candidates against a base vector: which (read, candidate) pairs are rescored, and their values.
// The stateless entry point composes its outputs from this on the host (its bits are pinned by its tests); a
// phmm_likelihood handle brings the base vector on the device and composes on the device.
struct CncJob {
    // in
    const uint32_t *base_cn = nullptr;  // host [N]
    const uint32_t *d_base = nullptr;   // the same vector on the device; nullptr: uploaded from base_cn
    uint64_t Tb = 0;                    // sum of e(base) over the emittable nodes
    uint32_t min_cn = 0, C = 0;
    const uint64_t *chg_off = nullptr;
    const uint32_t *chg_node = nullptr, *chg_cn = nullptr;
    const phmm_likelihood *grp = nullptr;  // chg_node holds group ids of this handle (uniform groups, checked by the caller)
    bool on_device = false;  // keep the read masks (WS_LK_MASKS) and every final value in the [D][R] planes (WS_OUT)
    // out
    std::vector<uint8_t> full;       // [C] no finite shift: every non-empty read is rescored
    std::vector<uint64_t> Tc;        // [C]
    std::vector<double> shift;       // [C] ln(Tb / Tc), 0 where full
    std::vector<uint64_t> n_resc;    // [C]
    std::vector<uint2> pairs;        // {read, slot}, read-major
    std::vector<uint32_t> cand_of, slot_of;
    std::vector<double> res;         // value per pair
    const unsigned long long *d_rmask = nullptr;  // on_device: [W][R] read masks
};

void cnc_score(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mp, CncJob &job) {
    hipStream_t s = current_stream();
    const uint64_t R = reads->R;
    const uint32_t N = m->N;
    const uint8_t *emis = m->emission.data();
    const uint32_t *base_cn = job.base_cn, min_cn = job.min_cn, C = job.C;
    const uint64_t *chg_off = job.chg_off;
    const uint32_t *chg_node = job.chg_node, *chg_cn = job.chg_cn;
    const uint64_t Tb = job.Tb;
    auto eff = [&](uint32_t k) { return std::max(k, min_cn); };
    const phmm_likelihood *grp = job.grp;
    const uint32_t G = grp ? grp->G : 0;
    const size_t S = grp ? (size_t)G + grp->P : N;  // entries of one word of the mask table

    // effective changes (e differs from the base) and T_c, exact in integers; in group units from the group table
    // alone: every node of a group holds g_cn, so d is the node form's d and the group adds d per emittable node
    std::vector<uint2> marks;  // {candidate, node or group}
    std::vector<uint8_t> &full = job.full;
    std::vector<double> &shift = job.shift;
    full.assign(C, 0);
    shift.assign(C, 0.0);
    job.Tc.assign(C, 0);
    for (uint32_t c = 0; c < C; c++) {
        int64_t dT = 0;
        for (uint64_t j = chg_off[c]; j < chg_off[c + 1]; j++) {
            const uint32_t v = chg_node[j];
            if (grp) {
                const int64_t d = (int64_t)eff(chg_cn[j]) - (int64_t)eff(grp->g_cn[v]);
                if (d == 0 || grp->g_off[v + 1] == grp->g_off[v]) continue;
                marks.push_back(make_uint2(c, v));
                dT += d * (int64_t)grp->g_emit[v];
                continue;
            }
            const int64_t d = (int64_t)eff(chg_cn[j]) - (int64_t)eff(base_cn[v]);
            if (d == 0) continue;
            marks.push_back(make_uint2(c, v));
            if (emis[v] != (uint8_t)'n') dT += d;
        }
        const uint64_t Tc = (uint64_t)((int64_t)Tb + dT);
        job.Tc[c] = Tc;
        full[c] = Tb == 0 || Tc == 0;  // (no finite shift: scored in full)
        if (!full[c]) shift[c] = std::log((double)Tb / (double)Tc);
    }

    trace("cnc: effective changes (host)");

    // read masks: bit c % 64 of word c / 64 set when the read's lists meet A_c
    const uint32_t W = (C + 63) / 64;
    std::vector<unsigned long long> rmask((size_t)W * R, 0ull);
    DevBuf &d_mask = ws(m, WS_CNC_MASKS), &d_list = ws(m, WS_CNC_LIST);
    DevBuf &d_nrmask = job.on_device ? ws(m, WS_LK_MASKS) : d_mask;  // (d_mask takes the pairs below)
    if (job.on_device) {
        d_nrmask.reserve((size_t)W * S * 8 + (size_t)W * R * 8);
        unsigned long long *rm = d_nrmask.as<unsigned long long>() + (size_t)W * S;
        if (marks.empty()) HIP_CHECK(hipMemsetAsync(rm, 0, (size_t)W * R * 8, s));
        job.d_rmask = rm;
    }
    if (!marks.empty()) {
        const size_t nm_bytes = (size_t)W * S * 8, rm_bytes = (size_t)W * R * 8;
        d_nrmask.reserve(nm_bytes + rm_bytes);
        d_list.reserve(marks.size() * sizeof(uint2));
        unsigned long long *nm = d_nrmask.as<unsigned long long>(), *rm = nm + (size_t)W * S;
        HIP_CHECK(hipMemsetAsync(nm, 0, nm_bytes, s));
        HIP_CHECK(hipMemcpyAsync(d_list.p, marks.data(), marks.size() * sizeof(uint2), hipMemcpyHostToDevice, s));
        if (grp) {
            hipLaunchKernelGGL(cng_mark, dim3((unsigned)((marks.size() + 255) / 256)), dim3(256), 0, s, d_list.as<uint2>(),
                               (uint32_t)marks.size(), grp->d_bp_off.as<uint32_t>(), grp->d_bp_slot.as<uint32_t>(), G,
                               (uint32_t)S, nm);
            hipLaunchKernelGGL(cng_read_mask, dim3((unsigned)((R + 3) / 4), W), dim3(256), 0, s,
                               reads->d_off.as<uint64_t>(), R, mp->d_pos_off.as<uint64_t>(), mp->d_nodes.as<uint32_t>(),
                               grp->d_g_slot.as<uint2>(), G, (uint32_t)S, (const unsigned long long *)nm, rm);
        } else {
            hipLaunchKernelGGL(cnc_mark, dim3((unsigned)((marks.size() + 255) / 256)), dim3(256), 0, s, d_list.as<uint2>(),
                               (uint32_t)marks.size(), m->dev.par_off.as<uint32_t>(), m->dev.par_node.as<uint32_t>(), N, nm);
            hipLaunchKernelGGL(cnc_read_mask, dim3((unsigned)((R + 3) / 4), W), dim3(256), 0, s, reads->d_off.as<uint64_t>(),
                               R, mp->d_pos_off.as<uint64_t>(), mp->d_nodes.as<uint32_t>(), N, nm, rm);
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(rmask.data(), rm, rm_bytes, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
    }

    trace("cnc: mark + read masks");

    // work list: (read, candidate) pairs, read-major, candidates ascending; slot = rank among the candidates with a pair
    std::vector<unsigned long long> fullw(W, 0ull);
    for (uint32_t c = 0; c < C; c++)
        if (full[c]) fullw[c >> 6] |= 1ull << (c & 63);
    std::vector<uint64_t> &n_resc = job.n_resc;
    n_resc.assign(C, 0);
    std::vector<uint2> &pairs = job.pairs;  // {read, candidate}, then {read, slot}
    pairs.clear();
    std::vector<uint64_t> read_pair_off(R + 1, 0);
    for (uint64_t r = 0; r < R; r++) {
        read_pair_off[r] = pairs.size();
        if (reads->off[r + 1] == reads->off[r]) continue;
        for (uint32_t w = 0; w < W; w++) {
            unsigned long long b = rmask[(size_t)w * R + r] | fullw[w];
            while (b) {
                const uint32_t c = w * 64 + (uint32_t)__builtin_ctzll(b);
                b &= b - 1;
                pairs.push_back(make_uint2((uint32_t)r, c));
                n_resc[c]++;
            }
        }
    }
    read_pair_off[R] = pairs.size();
    std::vector<uint32_t> &slot_of = job.slot_of, &cand_of = job.cand_of;
    slot_of.assign(C, 0xffffffffu);
    cand_of.clear();
    for (uint32_t c = 0; c < C; c++)
        if (n_resc[c]) {
            slot_of[c] = (uint32_t)cand_of.size();
            cand_of.push_back(c);
        }
    const uint32_t D = (uint32_t)cand_of.size();
    for (auto &q : pairs) q.y = slot_of[q.y];

    std::vector<double> &res = job.res;
    res.assign(pairs.size(), 0.0);
    trace("cnc: pair list (host)");
    EvTimer tm(timing_enabled());
    if (D) {
        // init / trans of the D dirty candidates: the base vector plus their changes, then the full form's cn_totals /
        // cn_probs -- the same probabilities, bit for bit
        DevBuf &staging = ws(m, WS_STAGING);
        std::vector<uint3> apply;
        for (uint32_t d = 0; d < D; d++)
            for (uint64_t j = chg_off[cand_of[d]]; j < chg_off[cand_of[d] + 1]; j++)
                apply.push_back(make_uint3(d, chg_node[j], chg_cn[j]));
        const size_t ni = (size_t)D * N;
        const size_t tot_at = (ni * sizeof(uint32_t) + 255) / 256 * 256;
        staging.reserve(tot_at + D * sizeof(unsigned long long));
        const size_t apply_at = ((size_t)N * sizeof(uint32_t) + 255) / 256 * 256;
        d_list.reserve(apply_at + std::max<size_t>(apply.size(), 1) * sizeof(uint3));
        const uint32_t *d_base = job.d_base ? job.d_base : d_list.as<uint32_t>();
        uint3 *d_apply = (uint3 *)(d_list.as<char>() + apply_at);
        uint32_t *d_cn = staging.as<uint32_t>();
        unsigned long long *d_tot = (unsigned long long *)(staging.as<char>() + tot_at);
        if (!job.d_base)
            HIP_CHECK(hipMemcpyAsync(d_list.p, base_cn, N * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        if (!apply.empty())
            HIP_CHECK(hipMemcpyAsync(d_apply, apply.data(), apply.size() * sizeof(uint3), hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemsetAsync(d_tot, 0, D * sizeof(unsigned long long), s));
        const unsigned nb = (unsigned)((N + 255) / 256);
        hipLaunchKernelGGL(cnc_expand, dim3(nb, D), dim3(256), 0, s, d_base, N, d_cn);
        if (!apply.empty() && grp)  // {slot, group, cn}
            hipLaunchKernelGGL(cng_apply, dim3((unsigned)apply.size()), dim3(256), 0, s, (const uint3 *)d_apply,
                               grp->d_g_off.as<uint64_t>(), grp->d_g_nodes.as<uint32_t>(), N, d_cn);
        else if (!apply.empty())
            hipLaunchKernelGGL(cnc_apply, dim3((unsigned)((apply.size() + 255) / 256)), dim3(256), 0, s,
                               (const uint3 *)d_apply, (uint32_t)apply.size(), N, d_cn);
        copy_num_probs(m, d_cn, D, min_cn, d_tot);
        trace("cnc: expand + cn_probs");

        // the pairs on the device, a value and an error word each behind them, and through the scheduler: the kernels
        // write [D][R] planes
        const size_t res_at = (pairs.size() * sizeof(uint2) + 255) / 256 * 256;
        const size_t rerr_at = res_at + (pairs.size() * sizeof(double) + 255) / 256 * 256;
        d_mask.reserve(rerr_at + pairs.size() * sizeof(uint32_t));  // (the masks are spent)
        HIP_CHECK(hipMemcpyAsync(d_mask.p, pairs.data(), pairs.size() * sizeof(uint2), hipMemcpyHostToDevice, s));
        HintedWork w;
        w.planes = D;
        w.call_cands = C;
        w.pair_off = read_pair_off.data();
        w.pairs = pairs.data();
        w.d_pairs = d_mask.as<uint2>();
        w.d_res = (double *)(d_mask.as<char>() + res_at);
        w.d_rerr = (uint32_t *)(d_mask.as<char>() + rerr_at);
        w.scatter_exact = job.on_device;
        w.vals = res.data();
        hinted_run(m, reads, mp,
                   hinted_args(m, reads, mp, D, ws(m, WS_CAND_INIT).as<double>(), ws(m, WS_CAND_TRANS).as<double>(), nullptr), w);
    }
    stats().ms[2] += tm.stop();  // (on top of the base pass; cells stay those of the base pass)
}

}  // namespace

void full_prob_reads_copy_num_changes(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mp,
                                      const uint32_t *base_cn, uint32_t min_cn, uint32_t C, const uint64_t *chg_off,
                                      const uint32_t *chg_node, const uint32_t *chg_cn, double *out_logp,
                                      double *out_total, uint64_t *out_n_rescored) {
    const uint64_t R = reads->R;
    const uint32_t N = m->N;
    const uint8_t *emis = m->emission.data();
    if (R == 0) {  // (an empty product: ln 1 per candidate, nothing rescored)
        const std::vector<double> z(C, 0.0);
        const std::vector<uint64_t> zn(C, 0);
        put_doubles(out_total, z.data(), C);
        put_bytes(out_n_rescored, zn.data(), (size_t)C * sizeof(uint64_t));
        return;
    }

    // the base: one call of the full form
    trace("cnc: enter");
    std::vector<double> base(R);
    double base_tot = 0.0;
    full_prob_reads_hinted(m, reads, mp, 1, nullptr, nullptr, base.data(), &base_tot, nullptr, base_cn, min_cn);

    trace("cnc: base pass");
    CncJob job;
    job.base_cn = base_cn;
    for (uint32_t v = 0; v < N; v++)
        if (emis[v] != (uint8_t)'n') job.Tb += std::max(base_cn[v], min_cn);
    job.min_cn = min_cn;
    job.C = C;
    job.chg_off = chg_off;
    job.chg_node = chg_node;
    job.chg_cn = chg_cn;
    trace("cnc: T_base (host sum)");
    cnc_score(m, reads, mp, job);
    const std::vector<uint8_t> &full = job.full;
    const std::vector<double> &shift = job.shift, &res = job.res;
    const std::vector<uint2> &pairs = job.pairs;

    // clean reads: base + ln(T_base / T_c); the rescored pairs over them; totals in read order, as the full form sums
    std::vector<double> out((size_t)C * R);
    std::vector<double> tot(C, 0.0);
    for (uint32_t c = 0; c < C; c++) {
        double *o = out.data() + (size_t)c * R;
        for (uint64_t r = 0; r < R; r++) o[r] = (full[c] || reads->off[r + 1] == reads->off[r]) ? base[r] : base[r] + shift[c];
    }
    for (size_t q = 0; q < pairs.size(); q++) out[(size_t)job.cand_of[pairs[q].y] * R + pairs[q].x] = res[q];
    for (uint32_t c = 0; c < C; c++)
        for (uint64_t r = 0; r < R; r++) tot[c] += out[(size_t)c * R + r];
    put_doubles(out_logp, out.data(), out.size());
    put_doubles(out_total, tot.data(), C);
    put_bytes(out_n_rescored, job.n_resc.data(), (size_t)C * sizeof(uint64_t));
    trace("cnc: compose [C][R] (host)");
}

// ---------------------------------------------------------------- phmm_likelihood: the sampler's state on the device
// The greedy search of sample_posterior (posterior.rs:314-417) at one k: score the neighbours of the current vector
// (sample_posterior_once, posterior.rs:470-528), move to one or to the union of several (posterior.rs:532-590), repeat.
// The handle keeps the vector and, per read, val[r] / T_at[r] (phmm_internal.h); a candidate batch is cnc_score against
// them with no base pass, and a move is cnc_score of one candidate whose results are written back.  DESIGN.md section 6.

struct LkCand {
    unsigned long long Tc;
    uint32_t slot;  // plane of the candidate's rescored reads in the [D][R] results
    uint32_t full;
};
// block c: out[c][r] = the plane's value where (c, r) was rescored, else val[r] + ln(T_at[r] / T_c); tot[c] = their sum,
// thread-strided partial sums reduced over a fixed tree (the same bits on every call).  rmask == nullptr: nothing rescored.
__global__ void __launch_bounds__(256) lk_compose(const LkCand *cand, const uint64_t *read_off, uint64_t R,
                                                  const double *val, const unsigned long long *tat,
                                                  const unsigned long long *rmask, const double *plane, double *out,
                                                  double *tot) {
    const uint32_t c = blockIdx.x;
    const LkCand k = cand[c];
    const unsigned long long *w = rmask ? rmask + (size_t)(c >> 6) * R : nullptr;
    double s = 0.0;
    for (uint64_t r = threadIdx.x; r < R; r += 256) {
        double v = val[r];
        if (read_off[r + 1] != read_off[r]) {
            if (k.full || (w && ((w[r] >> (c & 63)) & 1ull))) v = plane[(size_t)k.slot * R + r];
            else if (tat[r] != k.Tc) v += log((double)tat[r] / (double)k.Tc);
        }
        if (out) out[(size_t)c * R + r] = v;
        s += v;
    }
    __shared__ double sh[256];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) tot[c] = sh[0];
}
// a move: the reads it rescored take the plane's value and the T of the new vector
__global__ void __launch_bounds__(256) lk_commit(const uint64_t *read_off, uint64_t R, const unsigned long long *rmask,
                                                 uint32_t full, const double *plane, unsigned long long T_new,
                                                 double *val, unsigned long long *tat) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= R || read_off[r + 1] == read_off[r]) return;
    if (full || (rmask[r] & 1ull)) {
        val[r] = plane[r];
        tat[r] = T_new;
    }
}

namespace {

// values and total of the handle's state (or of a scored batch) through lk_compose, into WS_LK_COMPOSE: cand | tot | out
struct Composed {
    const double *tot, *out;
};
Composed lk_run_compose(const phmm_likelihood *lk, const std::vector<LkCand> &cand, const unsigned long long *rmask,
                        bool want_out) {
    hipStream_t s = current_stream();
    const uint64_t R = lk->reads->R;
    const size_t C = cand.size();
    DevBuf &buf = ws(lk->m, WS_LK_COMPOSE);
    const size_t tot_at = (C * sizeof(LkCand) + 255) / 256 * 256, out_at = tot_at + (C * sizeof(double) + 255) / 256 * 256;
    buf.reserve(out_at + (want_out ? C * R * sizeof(double) : 0));
    LkCand *d_cand = buf.as<LkCand>();
    double *d_tot = (double *)(buf.as<char>() + tot_at);
    double *d_o = want_out ? (double *)(buf.as<char>() + out_at) : nullptr;
    HIP_CHECK(hipMemcpyAsync(d_cand, cand.data(), C * sizeof(LkCand), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(lk_compose, dim3((unsigned)C), dim3(256), 0, s, (const LkCand *)d_cand,
                       lk->reads->d_off.as<uint64_t>(), R, (const double *)lk->d_val.as<double>(),
                       (const unsigned long long *)lk->d_tat.as<unsigned long long>(), rmask,
                       (const double *)ws(lk->m, WS_OUT).as<double>(), d_o, d_tot);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(s));  // (cand is the caller's)
    return Composed{d_tot, d_o};
}

void lk_prepare(const phmm_likelihood *lk) {
    upload_reads(lk->reads);
    upload_mappings(lk->mp);
    ensure_logib(lk->m, lk->reads->max_len + 1);
    stats() = CallStats();
}

}  // namespace

void likelihood_refresh(phmm_likelihood *lk) {
    const uint64_t R = lk->reads->R;
    uint64_t T = 0;
    for (uint32_t v = 0; v < lk->m->N; v++)
        if (lk->m->emission[v] != (uint8_t)'n') T += std::max(lk->cn[v], lk->min_cn);
    if (R) {
        std::vector<double> val(R);
        double tot = 0.0;
        full_prob_reads_hinted(lk->m, lk->reads, lk->mp, 1, nullptr, nullptr, val.data(), &tot, nullptr, lk->cn.data(),
                               lk->min_cn);
        const std::vector<unsigned long long> tat(R, T);
        hipStream_t s = current_stream();
        HIP_CHECK(hipMemcpyAsync(lk->d_val.p, val.data(), R * sizeof(double), hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(lk->d_tat.p, tat.data(), R * sizeof(unsigned long long), hipMemcpyHostToDevice, s));
        HIP_CHECK(hipStreamSynchronize(s));
    }
    lk->T = T;
}

void likelihood_score_changes(phmm_likelihood *lk, uint32_t C, const uint64_t *chg_off, const uint32_t *chg_node,
                              const uint32_t *chg_cn, double *out_logp, double *out_total, uint64_t *out_n_rescored,
                              bool by_group) {
    const uint64_t R = lk->reads->R;
    if (R == 0) {
        const std::vector<double> z(C, 0.0);
        const std::vector<uint64_t> zn(C, 0);
        put_doubles(out_total, z.data(), C);
        put_bytes(out_n_rescored, zn.data(), (size_t)C * sizeof(uint64_t));
        return;
    }
    lk_prepare(lk);
    trace("lk: enter");
    CncJob job;
    job.base_cn = lk->cn.data();
    job.d_base = lk->d_cn.as<uint32_t>();
    job.Tb = lk->T;
    job.min_cn = lk->min_cn;
    job.C = C;
    job.chg_off = chg_off;
    job.chg_node = chg_node;
    job.chg_cn = chg_cn;
    job.grp = by_group ? lk : nullptr;
    job.on_device = true;
    cnc_score(lk->m, lk->reads, lk->mp, job);

    std::vector<LkCand> cand(C);
    for (uint32_t c = 0; c < C; c++) cand[c] = LkCand{job.Tc[c], job.slot_of[c], job.full[c]};
    const Composed r = lk_run_compose(lk, cand, job.d_rmask, out_logp != nullptr);
    copy_out(out_logp, r.out, (size_t)C * R * sizeof(double));
    copy_out(out_total, r.tot, (size_t)C * sizeof(double));
    put_bytes(out_n_rescored, job.n_resc.data(), (size_t)C * sizeof(uint64_t));
    trace("lk: compose (device)");
}

namespace {
// a node-form move of nodes that lie in groups: a group all of whose nodes took one value follows it, a group whose
// changed nodes keep its value is untouched, any other becomes mixed.  O(changes).
void lk_groups_after_node_move(phmm_likelihood *lk, uint64_t n_chg, const uint32_t *chg_node, const uint32_t *chg_cn) {
    if (!lk->G) return;
    struct Touch {
        uint32_t g, n, val;
        bool one_val;
    };
    std::vector<Touch> touched;
    if (++lk->g_stamp == 0) {
        std::fill(lk->g_seen.begin(), lk->g_seen.end(), 0u);
        lk->g_stamp = 1;
    }
    std::vector<uint32_t> &at = lk->g_at;
    for (uint64_t j = 0; j < n_chg; j++) {
        const uint32_t g = lk->g_of[chg_node[j]];
        if (g == 0xffffffffu) continue;
        if (lk->g_seen[g] != lk->g_stamp) {
            lk->g_seen[g] = lk->g_stamp;
            at[g] = (uint32_t)touched.size();
            touched.push_back(Touch{g, 0, chg_cn[j], true});
        }
        Touch &t = touched[at[g]];
        t.n++;
        t.one_val = t.one_val && chg_cn[j] == t.val;
    }
    for (const Touch &t : touched) {
        if (t.one_val && t.n == lk->g_off[t.g + 1] - lk->g_off[t.g]) lk->g_cn[t.g] = t.val;
        else if (!(t.one_val && t.val == lk->g_cn[t.g])) lk->g_cn[t.g] = 0xffffffffu;
    }
}
}  // namespace

void likelihood_move(phmm_likelihood *lk, uint64_t n_chg, const uint32_t *chg_node, const uint32_t *chg_cn,
                     double *out_total, uint64_t *out_n_rescored, bool by_group) {
    hipStream_t s = current_stream();
    const uint64_t R = lk->reads->R;
    const uint32_t N = lk->m->N;
    uint64_t n_resc = 0;
    if (n_chg) {
        const uint64_t off[2] = {0, n_chg};
        CncJob job;
        job.base_cn = lk->cn.data();
        job.d_base = lk->d_cn.as<uint32_t>();
        job.Tb = lk->T;
        job.min_cn = lk->min_cn;
        job.C = 1;
        job.chg_off = off;
        job.chg_node = chg_node;
        job.chg_cn = chg_cn;
        job.grp = by_group ? lk : nullptr;
        job.on_device = true;
        uint64_t T_new = 0;
        if (R) {
            lk_prepare(lk);
            cnc_score(lk->m, lk->reads, lk->mp, job);
            T_new = job.Tc[0];
            n_resc = job.n_resc[0];
        } else {
            int64_t dT = 0;
            for (uint64_t j = 0; j < n_chg; j++)
                if (by_group)
                    dT += ((int64_t)std::max(chg_cn[j], lk->min_cn) - (int64_t)std::max(lk->g_cn[chg_node[j]], lk->min_cn)) *
                          (int64_t)lk->g_emit[chg_node[j]];
                else if (lk->m->emission[chg_node[j]] != (uint8_t)'n')
                    dT += (int64_t)std::max(chg_cn[j], lk->min_cn) - (int64_t)std::max(lk->cn[chg_node[j]], lk->min_cn);
            T_new = (uint64_t)((int64_t)lk->T + dT);
        }
        // the total under the new vector, before anything changes: the move's own planes and mask over the old state
        // (the bits phmm_likelihood_current returns afterwards: the same values reduced over the same tree)
        std::vector<uint3> apply(n_chg);
        for (uint64_t j = 0; j < n_chg; j++) apply[j] = make_uint3(0, chg_node[j], chg_cn[j]);
        DevBuf &d_apply = ws(lk->m, WS_LK_COMPOSE);
        d_apply.reserve(std::max<size_t>(apply.size() * sizeof(uint3), 512));  // (lk_run_compose's own need: no growth below)
        double total = 0.0;
        if (R) {
            const std::vector<LkCand> cand(1, LkCand{T_new, job.slot_of[0], job.full[0]});
            const Composed r = lk_run_compose(lk, cand, job.d_rmask, false);
            HIP_CHECK(hipMemcpyAsync(&total, r.tot, sizeof(double), hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipStreamSynchronize(s));
        }
        HIP_CHECK(hipMemcpyAsync(d_apply.p, apply.data(), apply.size() * sizeof(uint3), hipMemcpyHostToDevice, s));
        HIP_CHECK(hipStreamSynchronize(s));
        // everything that can fail is behind us: the state changes here, in stream order
        if (n_resc)
            hipLaunchKernelGGL(lk_commit, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, s,
                               lk->reads->d_off.as<uint64_t>(), R, job.d_rmask, (uint32_t)job.full[0],
                               (const double *)ws(lk->m, WS_OUT).as<double>(), (unsigned long long)T_new,
                               lk->d_val.as<double>(), lk->d_tat.as<unsigned long long>());
        if (by_group)
            hipLaunchKernelGGL(cng_apply, dim3((unsigned)apply.size()), dim3(256), 0, s, (const uint3 *)d_apply.as<uint3>(),
                               lk->d_g_off.as<uint64_t>(), lk->d_g_nodes.as<uint32_t>(), N, lk->d_cn.as<uint32_t>());
        else
            hipLaunchKernelGGL(cnc_apply, dim3((unsigned)((apply.size() + 255) / 256)), dim3(256), 0, s,
                               (const uint3 *)d_apply.as<uint3>(), (uint32_t)apply.size(), N, lk->d_cn.as<uint32_t>());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(s));
        if (by_group) {  // (the host mirror is written here only: scoring in group units reads g_cn)
            for (uint64_t j = 0; j < n_chg; j++) {
                const uint32_t g = chg_node[j];
                for (uint64_t i = lk->g_off[g]; i < lk->g_off[g + 1]; i++) lk->cn[lk->g_nodes[i]] = chg_cn[j];
                lk->g_cn[g] = chg_cn[j];
            }
        } else {
            lk_groups_after_node_move(lk, n_chg, chg_node, chg_cn);
            for (uint64_t j = 0; j < n_chg; j++) lk->cn[chg_node[j]] = chg_cn[j];
        }
        lk->T = T_new;
        put_doubles(out_total, &total, 1);
    } else if (out_total) {
        likelihood_current(lk, nullptr, nullptr, out_total);
    }
    put_bytes(out_n_rescored, &n_resc, sizeof(uint64_t));
}

void likelihood_current(const phmm_likelihood *lk, uint32_t *out_cn, double *out_logp, double *out_total) {
    const uint64_t R = lk->reads->R;
    if (out_cn && lk->m->N) std::memcpy(out_cn, lk->cn.data(), (size_t)lk->m->N * sizeof(uint32_t));
    if (!out_logp && !out_total) return;
    if (R == 0) {
        const double zero = 0.0;
        put_doubles(out_total, &zero, 1);
        return;
    }
    upload_reads(lk->reads);
    const std::vector<LkCand> cand(1, LkCand{lk->T, 0, 0});
    const Composed r = lk_run_compose(lk, cand, nullptr, out_logp != nullptr);
    copy_out(out_logp, r.out, R * sizeof(double));
    copy_out(out_total, r.tot, sizeof(double));
}


}  // namespace phmm

