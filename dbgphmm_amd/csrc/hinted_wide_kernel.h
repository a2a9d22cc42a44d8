// The score-only hinted forward (forward_with_mapping_score_only, src/hmmv2/forward.rs:79-89) for reads whose longest
// mapping list holds 65-400 nodes, on ONE BLOCK per (read, group of candidates): thread = list slot.
//
// hinted_score_kernel<128 / 400> walks such a column with one wave, 64 slots at a time, through the CSR and a link
// table in LDS, one wave per (read, candidate).  Here the recursion is the one of hinted_lean_kernel /
// hinted_packed_kernel (fwd_list_step, forward.rs:51-89, 337-388, 423-524, 554-558: fm, fi, fib, fd0 + n_max_gaps x
// fdt over mapping.nodes(i), non-adaptive, fe at the end) with a block in the place of the wave:
//   * a column lives in registers (m, i, d of the entry on its thread).  What other threads read of it goes through
//     LDS: G = p_MM m + p_IM i + p_DM d and H = p_MI m + p_II i + p_DI d of the previous column by ITS slots, and the
//     Del level values of the current column (two buffers, one barrier per level);
//   * the LDS holds two node -> slot tables (previous and current list).  Each thread resolves its node's in-list
//     parents in both and its own slot in the previous list ONCE per position, for every candidate of the block;
//   * per candidate only init[node], trans[edge] (through the packed ParRec: degree <= ADJ_DEG) and the arithmetic
//     differ -- the structure of hinted_packed_kernel.  A parent outside the list enters with weight 0;
//   * every operation on values is an HStep call.  The column's scale is the power of two of the block-wide maximum
//     (a maximum has no order), and the end sum has ONE association: wave_sum within each wave of 64 slots, then the
//     wave totals added in wave order by one thread.  Waves past the list hold zeros and x + 0 = x, so a 128-thread
//     and a 448-thread block give the same bits, and so does any candidate slot of any batch.
// A column more than 2^512 below its predecessor or a zero end sum gives -inf (the host sends the pair to
// hinted_exact_kernel, as for the other classes).  A duplicate node is SP_ERR_DUPLICATE, a list beyond the block
// SP_ERR_CAPACITY; the host hands any flagged read but a duplicate to the generic kernel.
//
// STORE (forward_with_mapping with stored columns, forward.rs:51-75; one candidate per block): every position also
// leaves a forward record in HintedArgs::pool, the layout hinted_lean_kernel writes and load_record<CAP> /
// wb_load_record read -- {n, na = n, E, 0}, ids padded to an even count, m[n] i[n] d[n] in list order, values in the
// column's own scale.  One thread allocates, the offset travels through LDS; a full pool is SP_ERR_POOL.  The
// flavours without it hold none of this (the statements are discarded at compile time).
//
// Included by sparse.hip behind HintedArgs / HStep.
#pragma once

namespace phmm {

template <int BS, int CPB> struct HintedWideShared {
    static constexpr int HASH = BS <= 128 ? 256 : 1024;  // load <= 0.5 / <= 0.39 (lists of up to 128 / 400 nodes)
    static constexpr int HASH_SHIFT = BS <= 128 ? 24 : 22;
    uint32_t hkey[2][HASH];  // node -> slot of the list of position parity
    uint16_t hslot[2][HASH];
    double G[CPB][BS], H[CPB][BS];  // previous column, by its slots
    double lv[2][CPB][BS];          // Del level values of the current column
    double red[CPB][8], fin[CPB][8];
    uint32_t err;
};
// LDS per block (the figures in the table of DESIGN.md section 6)
static_assert(sizeof(HintedWideShared<128, 1>) <= 8 * 1024 && sizeof(HintedWideShared<128, 4>) <= 20 * 1024 &&
                  sizeof(HintedWideShared<448, 1>) <= 28 * 1024 && sizeof(HintedWideShared<448, 2>) <= 42 * 1024,
              "hinted_wide_kernel LDS budget");

// Barrier between the LDS phases of a position.  Only LDS traffic is ordered: a __syncthreads() would also wait for
// every global load in flight (s_waitcnt vmcnt(0)), and the records / init / trans of the next position are requested
// across these barriers.
__device__ __forceinline__ void hw_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

template <int HASH> __device__ __forceinline__ int hw_find(const uint32_t *key, const uint16_t *slot, uint32_t h, uint32_t id) {
    for (;;) {
        const uint32_t k = key[h];
        if (k == id) return (int)slot[h];
        if (k == 0xffffffffu) return -1;
        h = (h + 1) & (HASH - 1);
    }
}

// Reads x candidates: grid (reads of the class, ceil(n_cand / CPB)), candidates blockIdx.y * CPB + c.
// PAIRS: a block takes a work unit {read, CPB candidate slots} of read_ids, 0xffffffff for an idle slot.  An idle
// slot computes nothing and writes nothing.
template <int BS, int CPB, bool PAIRS, bool STORE = false>
// (448 threads are 7 waves: at 4 waves per SIMD -- 128 VGPRs -- two such blocks share a CU, at 3 only one)
__global__ void __launch_bounds__(BS, BS > 128 ? 4 : 1) hinted_wide_kernel(const HintedArgs a, const uint32_t n_cand) {
    constexpr int NW = BS / 64;
    using Sh = HintedWideShared<BS, CPB>;
    constexpr int HASH = Sh::HASH;
    static_assert(BS % 64 == 0 && NW <= 8, "block shape");
    static_assert(!STORE || (CPB == 1 && !PAIRS), "a stored-column call is one candidate on the reads x candidates grid");
    __shared__ Sh sh;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const uint32_t *unit = a.read_ids + (size_t)blockIdx.x * (1 + CPB);
    const uint32_t rd = PAIRS ? unit[0] : a.read_ids[blockIdx.x];
    uint32_t cand[CPB];
    bool cand_ok[CPB];
    const double *init[CPB], *trans[CPB];
#pragma unroll
    for (int c = 0; c < CPB; c++) {
        if (PAIRS) {
            cand[c] = unit[1 + c];
            cand_ok[c] = cand[c] != 0xffffffffu;
            if (!cand_ok[c]) cand[c] = unit[1];
        } else {
            cand[c] = blockIdx.y * CPB + c;
            cand_ok[c] = cand[c] < n_cand;
            if (!cand_ok[c]) cand[c] = n_cand - 1;
        }
        // (an idle slot points at a live candidate: the requests below are unconditional)
        init[c] = a.init_c + (size_t)cand[c] * a.M.N;
        trans[c] = a.trans_c + (size_t)cand[c] * a.E;
    }
    const ParRec *prec = a.M.prec;
    const LinParams &lp = a.M.lp;
    const uint64_t b0 = a.read_off[rd];
    const int len = (int)(a.read_off[rd + 1] - b0);
    const uint64_t *po = a.map_pos_off + b0;
    uint32_t err = 0;
    // pipeline, as hinted_lean_kernel: offsets, node ids and the base two positions ahead, the record and the init
    // values one position ahead, trans[edge] as soon as the record is there
    uint64_t o_cur = po[0], o_nx = po[len >= 1 ? 1 : 0], o_n2 = po[len >= 2 ? 2 : (len >= 1 ? 1 : 0)];
    int n_cur = (int)(o_nx - o_cur), n_nx = (int)(o_n2 - o_nx);
    uint32_t id_cur = (t < n_cur && n_cur <= BS) ? a.map_nodes[o_cur + t] : 0u;
    uint32_t id_nx = (t < n_nx && n_nx <= BS) ? a.map_nodes[o_nx + t] : 0u;
    ParRec rc_cur = prec[id_cur];
    double in_cur[CPB], w_cur[CPB][ADJ_DEG];
#pragma unroll
    for (int c = 0; c < CPB; c++) {
        in_cur[c] = init[c][id_cur];
#pragma unroll
        for (int q = 0; q < ADJ_DEG; q++) w_cur[c][q] = q < (int)rc_cur.npar ? trans[c][rc_cur.pedge[q]] : 0.0;
    }
    uint8_t x_cur = len >= 1 ? a.bases[b0] : (uint8_t)0, x_nx = len >= 2 ? a.bases[b0 + 1] : (uint8_t)0;
    double pm[CPB], pi[CPB], pd[CPB], ibs[CPB];
    int Eprev[CPB];
    bool collapse[CPB];
#pragma unroll
    for (int c = 0; c < CPB; c++) {
        pm[c] = pi[c] = pd[c] = ibs[c] = 0.0;
        Eprev[c] = 0;
        collapse[c] = false;
    }
    for (int h = t; h < 2 * HASH; h += BS) (&sh.hkey[0][0])[h] = 0xffffffffu;
    if (t == 0) sh.err = 0;
    hw_sync();
    int n_prev = 0;
    for (int pos = 0; pos < len; pos++) {
        if (n_cur > BS) {  // (block-uniform)
            err |= SP_ERR_CAPACITY;
            break;
        }
        // ---- requests for the positions ahead
        const ParRec rc_nx = prec[id_nx];
        double in_nx[CPB];
#pragma unroll
        for (int c = 0; c < CPB; c++) in_nx[c] = init[c][id_nx];
        const uint64_t o_n3 = po[pos + 3 <= len ? pos + 3 : len];
        const int n_n2 = pos + 2 < len ? (int)(o_n3 - o_n2) : 0;
        const uint32_t id_n2 = (t < n_n2 && n_n2 <= BS) ? a.map_nodes[o_n2 + t] : 0u;
        const uint8_t x_n2 = pos + 2 < len ? a.bases[b0 + pos + 2] : (uint8_t)0;
        // ---- node -> slot table of this position's list (cleared behind the lookups of the position before last)
        const bool first = pos == 0;
        const int n = n_cur;
        const bool has = t < n;
        uint32_t *kc = sh.hkey[pos & 1], *kp = sh.hkey[(pos + 1) & 1];
        uint16_t *sc_ = sh.hslot[pos & 1];
        const uint16_t *sp_ = sh.hslot[(pos + 1) & 1];
        if (has) {
            uint32_t h = (id_cur * 2654435761u) >> Sh::HASH_SHIFT;
            for (;;) {
                const uint32_t old = atomicCAS(&kc[h], 0xffffffffu, id_cur);
                if (old == 0xffffffffu) {
                    sc_[h] = (uint16_t)t;
                    break;
                }
                if (old == id_cur) {
                    err |= SP_ERR_DUPLICATE;
                    break;
                }
                h = (h + 1) & (HASH - 1);
            }
        }
        hw_sync();
        // ---- the topology of the position, once for every candidate: slots of the in-list parents in the previous
        // (ps) and the current (cs) list, own slot in the previous list (os)
        int ps[ADJ_DEG], cs[ADJ_DEG];
        uint32_t anyq = 0;  // wave-uniform: some lane has a q-th parent
#pragma unroll
        for (int q = 0; q < ADJ_DEG; q++) {
            const bool use = has && q < (int)rc_cur.npar;
            ps[q] = cs[q] = -1;
            if (__ballot(use) != 0ull) {
                anyq |= 1u << q;
                if (use) {
                    const uint32_t h = (rc_cur.par[q] * 2654435761u) >> Sh::HASH_SHIFT;
                    if (!first) ps[q] = hw_find<HASH>(kp, sp_, h, rc_cur.par[q]);
                    cs[q] = hw_find<HASH>(kc, sc_, h, rc_cur.par[q]);
                }
            }
        }
        const int os = (has && !first) ? hw_find<HASH>(kp, sp_, (id_cur * 2654435761u) >> Sh::HASH_SHIFT, id_cur) : -1;
        const double pe = rc_cur.emis == x_cur ? lp.p_match : lp.p_mismatch;
        // ---- per candidate: fm, fi (forward.rs:337-388), fib (541-545), level-0 input of the Del closure
        double m[CPB], ii[CPB], d[CPB], ib_cur[CPB], c_del[CPB], wc[CPB][ADJ_DEG];
#pragma unroll
        for (int c = 0; c < CPB; c++) {
            m[c] = ii[c] = d[c] = ib_cur[c] = c_del[c] = 0.0;
            if (!cand_ok[c]) continue;
            const double c_begin = HStep::c_begin(lp, first, ibs[c]);
            ib_cur[c] = HStep::ib_cur(lp, first, ibs[c]);
            c_del[c] = __dmul_rn(lp.p_ID, ib_cur[c]);
            double acc = 0.0;
#pragma unroll
            for (int q = 0; q < ADJ_DEG; q++) {
                wc[c][q] = cs[q] >= 0 ? w_cur[c][q] : 0.0;
                if (!(anyq & (1u << q))) continue;
                const double wp = ps[q] >= 0 ? w_cur[c][q] : 0.0;
                acc = HStep::acc(wp, ps[q] >= 0 ? sh.G[c][ps[q]] : 0.0, acc);
            }
            const double hv = os >= 0 ? sh.H[c][os] : 0.0;
            m[c] = has ? HStep::match(pe, acc, in_cur[c], c_begin) : 0.0;
            ii[c] = (has && os >= 0) ? __dmul_rn(lp.p_random, hv) : 0.0;
            sh.lv[0][c][t] = HStep::lv(lp, m[c], ii[c]);
        }
        hw_sync();
        // (every lookup in the previous list's table is done: it is the table of the next position)
        for (int h = t; h < HASH; h += BS) kp[h] = 0xffffffffu;
        // weights of the next position (its record has arrived)
        double w_nx[CPB][ADJ_DEG];
        {
            int npmax = (int)rc_nx.npar;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) npmax = max(npmax, __shfl_xor(npmax, off));
            npmax = __builtin_amdgcn_readfirstlane(npmax);
#pragma unroll
            for (int c = 0; c < CPB; c++)
#pragma unroll
                for (int q = 0; q < ADJ_DEG; q++) {
                    if (q < npmax) w_nx[c][q] = q < (int)rc_nx.npar ? trans[c][rc_nx.pedge[q]] : 0.0;
                    else w_nx[c][q] = 0.0;
                }
        }
        // ---- fd0 + n_max_gaps x fdt restricted to the list (forward.rs:423-524): level t reads buffer t & 1
        for (int lvl = 0; lvl <= lp.n_max_gaps; lvl++) {
#pragma unroll
            for (int c = 0; c < CPB; c++) {
                if (!cand_ok[c]) continue;
                double sacc = 0.0;
#pragma unroll
                for (int q = 0; q < ADJ_DEG; q++) {
                    if (!(anyq & (1u << q))) continue;
                    sacc = HStep::acc(wc[c][q], cs[q] >= 0 ? sh.lv[lvl & 1][c][cs[q]] : 0.0, sacc);
                }
                sacc = lvl == 0 ? __fma_rn(in_cur[c], c_del[c], sacc) : __dmul_rn(sacc, lp.p_DD);
                sacc = has ? sacc : 0.0;
                d[c] = __dadd_rn(d[c], sacc);
                if (lvl < lp.n_max_gaps) sh.lv[(lvl + 1) & 1][c][t] = sacc;
            }
            if (lvl < lp.n_max_gaps) hw_sync();
        }
        // ---- rescale so that the column maximum of each candidate is in [0.5, 1)
#pragma unroll
        for (int c = 0; c < CPB; c++) {
            if (!cand_ok[c]) continue;
            const double v = wave_max(has ? fmax(fmax(m[c], ii[c]), d[c]) : 0.0);
            if (lane == 0) sh.red[c][wv] = v;
        }
        hw_sync();
#pragma unroll
        for (int c = 0; c < CPB; c++) {
            if (!cand_ok[c]) continue;
            double mx = ib_cur[c];
#pragma unroll
            for (int w = 0; w < NW; w++) mx = fmax(mx, sh.red[c][w]);
            const int e = sp_exp_of(mx);
            collapse[c] |= !first && e < HINT_COLLAPSE_EXP;
            const double sc = sp_pow2(-e);
            pm[c] = __dmul_rn(m[c], sc);
            pi[c] = __dmul_rn(ii[c], sc);
            pd[c] = __dmul_rn(d[c], sc);
            Eprev[c] = (first ? 0 : Eprev[c]) + e;
            ibs[c] = __dmul_rn(ib_cur[c], sc);
            // what the next position reads of this column
            if (has) {
                sh.G[c][t] = HStep::lin3(lp.p_MM, pm[c], lp.p_IM, pi[c], lp.p_DM, pd[c]);
                sh.H[c][t] = HStep::lin3(lp.p_MI, pm[c], lp.p_II, pi[c], lp.p_DI, pd[c]);
            }
        }
        if constexpr (STORE) {
            // ---- forward record of the position (every entry carries m, i and d; slot t = entry t)
            __shared__ unsigned long long rec_o;
            const uint64_t idb = (uint64_t)((n + 1) & ~1) * 4;
            const uint64_t bytes = 16 + idb + (uint64_t)(3 * n) * 8;
            if (t == 0) rec_o = atomicAdd(a.pool.top, (unsigned long long)bytes);
            hw_sync();
            const uint64_t o = rec_o;
            if (o + bytes > a.pool.cap) {  // (block-uniform: every thread read the same offset)
                err |= SP_ERR_POOL;
                break;
            }
            uint8_t *rec = a.pool.base + o;
            if (t == 0) {
                ((uint32_t *)rec)[0] = (uint32_t)n;
                ((uint32_t *)rec)[1] = (uint32_t)n;
                ((int *)rec)[2] = Eprev[0];
                ((uint32_t *)rec)[3] = 0;
                a.pool.off[b0 + pos] = o + 8;
            }
            if (has) {
                ((uint32_t *)(rec + 16))[t] = id_cur;
                double *om = (double *)(rec + 16 + idb);
                om[t] = pm[0];
                om[n + t] = pi[0];
                om[2 * n + t] = pd[0];
            }
        }
        // ---- the column becomes the previous one
        n_prev = n;
#pragma unroll
        for (int c = 0; c < CPB; c++) {
            in_cur[c] = in_nx[c];
#pragma unroll
            for (int q = 0; q < ADJ_DEG; q++) w_cur[c][q] = w_nx[c][q];
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
    if (err) atomicOr(&sh.err, err);
    // fe (forward.rs:554-558) of the last column, per candidate: wave sums, then the waves in order
#pragma unroll
    for (int c = 0; c < CPB; c++) {
        const double s = wave_sum(t < n_prev ? __dadd_rn(__dadd_rn(pm[c], pi[c]), pd[c]) : 0.0);
        if (lane == 0) sh.fin[c][wv] = s;
    }
    hw_sync();
    if (t == 0) {
        const uint32_t e_all = sh.err;
#pragma unroll
        for (int c = 0; c < CPB; c++) {
            if (!cand_ok[c]) continue;
            double stot = sh.fin[c][0];
#pragma unroll
            for (int w = 1; w < NW; w++) stot = __dadd_rn(stot, sh.fin[c][w]);
            const double lpv = e_all ? NAN : (collapse[c] ? -INFINITY : HStep::log_end(lp, stot, Eprev[c]));
            a.out_logp[(size_t)cand[c] * a.R + rd] = lpv;
            a.err[(size_t)cand[c] * a.R + rd] = e_all;
        }
    }
}

}  // namespace phmm
