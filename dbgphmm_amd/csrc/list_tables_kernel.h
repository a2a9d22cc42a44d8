// The tables of the list pass themselves (phmm_run_with_mapping_tables, include/phmm_amd_tables.h):
// forward_with_mapping (forward.rs:51-75) and backward_with_mapping (backward.rs:59-93) with every column written out.
//
// list_tables_forward_kernel<CAP, LPN> / list_tables_backward_kernel<CAP>: one wave64 per read, the column of the previous
// and of the current position in LDS (Col<CAP>, sparse_dev.h), the two capacity classes of every list call (longest list
// <= 64, <= 400).  Per position: the column step of the list pass (fwd_list_step / bwd_list_step, unchanged), then
// ln(value) + E ln 2 of every entry (E: the column's power-of-two exponent) and the column's two scalars.  The forward
// InsBegin is the chain SparseModel::logib; the backward begin states are what bwd_list_step returns.
//
// A column is kept as values times ONE power of two.  Two things fall out of that range on a read that crosses a k-mer of
// copy number 0 (test_oracle_edge_semantics.py), where for hundreds of bases the begin chain -- shrinking by p_random p_II
// per base -- is all that is left of the read:
//   backward: the columns before the cut are zero in every entry, so they have no scale of their own and the chain would
//     slide out of the double range in their frozen one.  The kernel re-seats the exponent of a zero column on its begin
//     states; no value changes, since 0 * 2^E is 0 for every E.
//   forward: behind the cut the path re-enters from the chain, thousands of bits under the dying values it shares a column
//     with; one exponent per column cannot hold both, and what the re-entry grows into is the read's whole probability.
//     The scaled kernel notices when it happens -- a column 2^-512 below the one before it, as in the list pass
//     (hinted_score_kernel), or a zero column beside a chain that is lost under the scale -- and reports LT_ERR_RANGE; the
//     host runs that read again in list_tables_forward_wide_kernel, the same recursion with an exponent per VALUE (the
//     arithmetic of the list pass's hinted_exact_kernel, restated here with the outputs).
#pragma once

#include "sparse_dyn.h"

namespace phmm {

struct ListTablesArgs {
    SparseModel M;
    const uint8_t *bases;
    const uint64_t *read_off;     // [R+1]
    const uint64_t *map_pos_off;  // [total_bases+1]
    const uint32_t *map_nodes;
    const uint32_t *read_ids;     // the reads of this launch
    // this half's outputs: values of entry a at ent[3 (a - ent0)], scalars of base g at scal[2 (g - row0)]; either may be
    // null.  A caller's device buffer has ent0 = row0 = 0; a staging buffer starts at the chunk's first entry / base.
    double *ent, *scal;
    uint64_t ent0, row0;
    double *logp;   // [R]
    uint32_t *err;  // [R]
};

// a private error bit beside SP_ERR_*: the scaled forward lost range on this read, run it in the wide-range kernel
static constexpr uint32_t LT_ERR_RANGE = 0x100u;
// a rescale exponent below this in ONE position (HINT_COLLAPSE_EXP of the list pass)
static constexpr int LT_COLLAPSE_EXP = -512;
// InsBegin of the previous column this far (natural log) below the column's scale: its products with init and the
// parameters are denormal or 0
static constexpr double LT_CHAIN_LOST = -600.0;

// fwd_list_step sets its error bits on the lanes that met them: the same bits on every lane, so that the loop over the
// positions ends for the whole wave at once
__device__ __forceinline__ uint32_t lt_wave_or(uint32_t e) {
    if (__ballot(e != 0) == 0) return 0u;
    for (int off = 32; off >= 1; off >>= 1) e |= (uint32_t)__shfl_xor((int)e, off);
    return e;
}

template <int CAP, int LPN>
__global__ void __launch_bounds__(64) list_tables_forward_kernel(const ListTablesArgs a) {
    __shared__ Col<CAP> cols[2];
    __shared__ int16_t lnk_slot[CAP * LPN];
    __shared__ double lnk_w[CAP * LPN];
    __shared__ double dA[CAP], dB[CAP];
    const int lane = threadIdx.x;
    const uint32_t rd = a.read_ids[blockIdx.x];
    const SparseModel &M = a.M;
    const uint64_t b0 = a.read_off[rd];
    const int len = (int)(a.read_off[rd + 1] - b0);
    uint32_t err = 0;
    if (lane == 0) {
        cols[0].n = cols[0].na = 0;
        cols[0].E = 0;
        cols[1].n = cols[1].na = 0;
        cols[1].E = 0;
    }
    wave_sync();
    double le = -INFINITY;  // ln F.tables[pos].e of the column computed last
    for (int pos = 0; pos < len && !err; pos++) {
        const uint64_t o0 = a.map_pos_off[b0 + pos];
        const int n = (int)(a.map_pos_off[b0 + pos + 1] - o0);
        if (n > CAP) {
            err |= SP_ERR_CAPACITY;
            break;
        }
        Col<CAP> &prev = cols[(pos + 1) & 1];
        Col<CAP> &cur = cols[pos & 1];
        const uint8_t x = a.bases[b0 + pos];
        err |= lt_wave_or(fwd_list_step<CAP, LPN>(M, prev, cur, a.map_nodes + o0, n, x, pos == 0, pos, lnk_slot, lnk_w, dA, dB));
        if (err) break;
        if (pos > 0) {
            const int Ep = prev.E;
            bool lost = cur.E - Ep < LT_COLLAPSE_EXP;
            const double lib = M.logib[pos - 1];
            if (!lost && lib > -INFINITY && lib - (double)Ep * SP_LN2 < LT_CHAIN_LOST) {
                // the chain is lost under the scale: harmless while the column lives, but a zero column is fed by it alone
                bool nz = false;
                for (int j = lane; j < n; j += 64) nz |= cur.m[j] != 0.0 || cur.i[j] != 0.0 || cur.d[j] != 0.0;
                lost = __ballot(nz) == 0;
            }
            if (lost) {
                err |= LT_ERR_RANGE;
                break;
            }
        }
        const double Eln = (double)cur.E * SP_LN2;
        if (a.ent) {
            double *o = a.ent + 3 * (o0 - a.ent0);
            for (int j = lane; j < n; j += 64) {
                o[3 * j + 0] = log(cur.m[j]) + Eln;
                o[3 * j + 1] = log(cur.i[j]) + Eln;
                o[3 * j + 2] = log(cur.d[j]) + Eln;
            }
        }
        le = col_log_end(M, cur);
        if (a.scal && lane == 0) {
            double *o = a.scal + 2 * (b0 + (uint64_t)pos - a.row0);
            o[0] = M.logib[pos];
            o[1] = le;
        }
    }
    for (int off = 32; off >= 1; off >>= 1) err |= (uint32_t)__shfl_xor((int)err, off);
    if (lane == 0) {
        a.logp[rd] = err ? NAN : le;
        a.err[rd] = err;
    }
}

// ---- the wide-range forward: every value carries its own binary exponent (a double mantissa in [0.5, 1) or 0, an int
// exponent), so nothing underflows whatever its distance from the column's best value
struct LtX {
    double m;
    int e;
};
__device__ __forceinline__ LtX ltx_norm(double v, int e) {
    if (v == 0.0) return LtX{0.0, 0};
    int k;
    const double m = frexp(v, &k);
    return LtX{m, e + k};
}
__device__ __forceinline__ LtX ltx_mul(LtX a, double p) { return ltx_norm(a.m * p, a.e); }
__device__ __forceinline__ LtX ltx_add(LtX a, LtX b) {
    if (a.m == 0.0) return b;
    if (b.m == 0.0) return a;
    if (a.e < b.e) {
        const LtX t = a;
        a = b;
        b = t;
    }
    const int d = b.e - a.e;
    if (d < -1000) return a;
    return ltx_norm(a.m + ldexp(b.m, d), a.e);
}
__device__ __forceinline__ double ltx_log(LtX a) { return a.m == 0.0 ? -INFINITY : log(a.m) + (double)a.e * SP_LN2; }

template <int XCAP, int XHASH> struct LtXCol {
    uint32_t id[XCAP];
    double m[XCAP], i[XCAP], d[XCAP];
    int me[XCAP], ie[XCAP], de[XCAP];
    uint32_t hkey[XHASH];
    uint16_t hval[XHASH];
};
template <int XCAP, int XHASH> __device__ __forceinline__ int ltx_find(const LtXCol<XCAP, XHASH> &c, uint32_t key) {
    uint32_t h = ((key * 2654435761u) >> 16) & (XHASH - 1);
    for (;;) {
        const uint32_t k = c.hkey[h];
        if (k == key) return (int)c.hval[h];
        if (k == H_EMPTY) return -1;
        h = (h + 1) & (XHASH - 1);
    }
}

template <int XCAP, int XHASH>
__global__ void __launch_bounds__(64) list_tables_forward_wide_kernel(const ListTablesArgs a) {
    typedef LtXCol<XCAP, XHASH> XCol;
    static_assert(XHASH >= 2 * XCAP && (XHASH & (XHASH - 1)) == 0, "hash at half load at most");
    __shared__ XCol cols[2];
    __shared__ double ta[XCAP], tb[XCAP];
    __shared__ int tae[XCAP], tbe[XCAP];
    const int lane = threadIdx.x;
    const uint32_t rd = a.read_ids[blockIdx.x];
    const SparseModel &M = a.M;
    const LinParams &lp = M.lp;
    const uint64_t b0 = a.read_off[rd];
    const int len = (int)(a.read_off[rd + 1] - b0);
    LtX mb = ltx_norm(1.0, 0), ib = LtX{0.0, 0};  // f_init (forward.rs:255-266)
    int np = 0, cur = 0;
    uint32_t err = 0;
    double le = -INFINITY;
    for (int pos = 0; pos < len; pos++, cur ^= 1) {
        XCol &Cc = cols[cur];
        const XCol &P = cols[cur ^ 1];
        const uint64_t e0 = a.map_pos_off[b0 + pos];
        const int n = (int)(a.map_pos_off[b0 + pos + 1] - e0);
        if (n > XCAP) {
            err |= SP_ERR_CAPACITY;
            break;
        }
        const uint8_t x = a.bases[b0 + pos];
        for (int h = lane; h < XHASH; h += 64) Cc.hkey[h] = H_EMPTY;
        wave_sync();
        bool dup = false;
        for (int j = lane; j < n; j += 64) {
            const uint32_t k = a.map_nodes[e0 + j];
            Cc.id[j] = k;
            uint32_t h = ((k * 2654435761u) >> 16) & (XHASH - 1);
            for (;;) {
                const uint32_t old = atomicCAS(&Cc.hkey[h], H_EMPTY, k);
                if (old == H_EMPTY) {
                    Cc.hval[h] = (uint16_t)j;
                    break;
                }
                if (old == k) {
                    dup = true;
                    break;
                }
                h = (h + 1) & (XHASH - 1);
            }
        }
        if (__ballot(dup) != 0) {
            err |= SP_ERR_DUPLICATE;
            break;
        }
        wave_sync();
        // fm, fi from the previous column (empty at pos 0)
        const LtX beg_m = ltx_add(ltx_mul(mb, lp.p_MM), ltx_mul(ib, lp.p_IM));
        for (int j = lane; j < n; j += 64) {
            const uint32_t k = Cc.id[j];
            LtX from_normal{0.0, 0};
            for (uint32_t e = M.par_off[k]; e < M.par_off[k + 1]; e++) {
                const int q = np > 0 ? ltx_find(P, M.par_node[e]) : -1;
                if (q < 0) continue;
                const LtX inner = ltx_add(ltx_add(ltx_mul(LtX{P.m[q], P.me[q]}, lp.p_MM), ltx_mul(LtX{P.i[q], P.ie[q]}, lp.p_IM)),
                                          ltx_mul(LtX{P.d[q], P.de[q]}, lp.p_DM));
                from_normal = ltx_add(from_normal, ltx_mul(inner, M.trans[M.par_edge[e]]));
            }
            const LtX mv = ltx_mul(ltx_add(from_normal, ltx_mul(beg_m, M.init[k])), M.emis[k] == x ? lp.p_match : lp.p_mismatch);
            Cc.m[j] = mv.m;
            Cc.me[j] = mv.e;
            const int me = np > 0 ? ltx_find(P, k) : -1;
            LtX iv{0.0, 0};
            if (me >= 0)
                iv = ltx_mul(ltx_add(ltx_add(ltx_mul(LtX{P.m[me], P.me[me]}, lp.p_MI), ltx_mul(LtX{P.i[me], P.ie[me]}, lp.p_II)),
                                     ltx_mul(LtX{P.d[me], P.de[me]}, lp.p_DI)),
                             lp.p_random);
            Cc.i[j] = iv.m;
            Cc.ie[j] = iv.e;
        }
        ib = ltx_mul(ltx_add(ltx_mul(mb, lp.p_MI), ltx_mul(ib, lp.p_II)), lp.p_random);  // fib; fmb = 0
        mb = LtX{0.0, 0};
        wave_sync();
        // fd0 from this column's m, i; then the Del levels over the same list
        const LtX beg_d = ltx_mul(ib, lp.p_ID);  // (mb = 0)
        for (int j = lane; j < n; j += 64) {
            const uint32_t k = Cc.id[j];
            LtX from_normal{0.0, 0};
            for (uint32_t e = M.par_off[k]; e < M.par_off[k + 1]; e++) {
                const int q = ltx_find(Cc, M.par_node[e]);
                if (q < 0) continue;
                const LtX g = ltx_add(ltx_mul(LtX{Cc.m[q], Cc.me[q]}, lp.p_MD), ltx_mul(LtX{Cc.i[q], Cc.ie[q]}, lp.p_ID));
                from_normal = ltx_add(from_normal, ltx_mul(g, M.trans[M.par_edge[e]]));
            }
            const LtX v = ltx_add(from_normal, ltx_mul(beg_d, M.init[k]));
            ta[j] = v.m;
            tae[j] = v.e;
            Cc.d[j] = v.m;
            Cc.de[j] = v.e;
        }
        double *src = ta, *dst = tb;
        int *srce = tae, *dste = tbe;
        for (int t = 0; t < lp.n_max_gaps; t++) {
            wave_sync();
            for (int j = lane; j < n; j += 64) {
                const uint32_t k = Cc.id[j];
                LtX sacc{0.0, 0};
                for (uint32_t e = M.par_off[k]; e < M.par_off[k + 1]; e++) {
                    const int q = ltx_find(Cc, M.par_node[e]);
                    if (q < 0) continue;
                    sacc = ltx_add(sacc, ltx_mul(LtX{src[q], srce[q]}, M.trans[M.par_edge[e]] * lp.p_DD));
                }
                dst[j] = sacc.m;
                dste[j] = sacc.e;
                const LtX dv = ltx_add(LtX{Cc.d[j], Cc.de[j]}, sacc);
                Cc.d[j] = dv.m;
                Cc.de[j] = dv.e;
            }
            double *tmp = src;
            src = dst;
            dst = tmp;
            int *tmpe = srce;
            srce = dste;
            dste = tmpe;
        }
        wave_sync();
        // the column's outputs: every entry, and fe (forward.rs:554-558) over the list
        LtX tot{0.0, 0};
        double *o = a.ent ? a.ent + 3 * (e0 - a.ent0) : nullptr;
        for (int j = lane; j < n; j += 64) {
            const LtX vm{Cc.m[j], Cc.me[j]}, vi{Cc.i[j], Cc.ie[j]}, vd{Cc.d[j], Cc.de[j]};
            tot = ltx_add(tot, ltx_add(ltx_add(vm, vi), vd));
            if (o) {
                o[3 * j + 0] = ltx_log(vm);
                o[3 * j + 1] = ltx_log(vi);
                o[3 * j + 2] = ltx_log(vd);
            }
        }
        for (int off = 32; off >= 1; off >>= 1) {
            LtX t;
            t.m = __shfl_xor(tot.m, off);
            t.e = __shfl_xor(tot.e, off);
            tot = ltx_add(tot, t);
        }
        le = ltx_log(ltx_mul(tot, lp.p_end));
        if (a.scal && lane == 0) {
            double *s = a.scal + 2 * (b0 + (uint64_t)pos - a.row0);
            s[0] = M.logib[pos];
            s[1] = le;
        }
        np = n;
    }
    if (lane == 0) {
        a.logp[rd] = err ? NAN : le;
        a.err[rd] = err;
    }
}

template <int CAP> __global__ void __launch_bounds__(64) list_tables_backward_kernel(const ListTablesArgs a) {
    __shared__ Col<CAP> cols[2];
    __shared__ double dA[CAP], dB[CAP];
    const int lane = threadIdx.x;
    const uint32_t rd = a.read_ids[blockIdx.x];
    const SparseModel &M = a.M;
    const uint64_t b0 = a.read_off[rd];
    const int len = (int)(a.read_off[rd + 1] - b0);
    uint32_t err = 0;
    if (lane == 0) {
        cols[0].n = cols[0].na = 0;
        cols[0].E = 0;
        cols[1].n = cols[1].na = 0;
        cols[1].E = 0;
    }
    wave_sync();
    double ib = 0.0;         // InsBegin of B.tables[pos+1] in that column's scale (b_init: 0)
    double lmb = -INFINITY;  // ln B.tables[pos].mb of the column computed last
    for (int pos = len - 1; pos >= 0 && !err; pos--) {
        const uint64_t o0 = a.map_pos_off[b0 + pos];
        const int n = (int)(a.map_pos_off[b0 + pos + 1] - o0);
        if (n > CAP) {
            err |= SP_ERR_CAPACITY;
            break;
        }
        Col<CAP> &prev = cols[(pos + 1) & 1];
        Col<CAP> &cur = cols[pos & 1];
        BeginStates bs = bwd_list_step<CAP>(M, prev, pos == len - 1, cur, a.map_nodes + o0, n, a.bases[b0 + pos], dA, dB, ib);
        int E = cur.E;
        const double Eln = (double)E * SP_LN2;
        double *o = a.ent ? a.ent + 3 * (o0 - a.ent0) : nullptr;
        bool nz = false, dup = false;
        for (int j = lane; j < n; j += 64) {
            const double vm = cur.m[j], vi = cur.i[j], vd = cur.d[j];
            nz |= vm != 0.0 || vi != 0.0 || vd != 0.0;
            dup |= hash_find(cur, cur.id[j]) != j;  // (bwd_list_step keeps the first entry of a node and says nothing)
            if (o) {
                o[3 * j + 0] = log(vm) + Eln;
                o[3 * j + 1] = log(vi) + Eln;
                o[3 * j + 2] = log(vd) + Eln;
            }
        }
        if (__ballot(dup) != 0) err |= SP_ERR_DUPLICATE;
        if (__ballot(nz) == 0) {
            // a zero column: its exponent follows the begin states, which are all that is left of the read's suffix
            const int e = sp_exp_of(fmax(bs.ib, bs.mb));
            if (e != 0) {
                const double s = sp_pow2(-e);
                bs.ib *= s;
                bs.mb *= s;
                E += e;
                wave_sync();
                if (lane == 0) cur.E = E;
                wave_sync();
            }
        }
        ib = bs.ib;
        lmb = log(bs.mb) + (double)E * SP_LN2;
        if (a.scal && lane == 0) {
            double *s = a.scal + 2 * (b0 + (uint64_t)pos - a.row0);
            s[0] = lmb;
            s[1] = log(bs.ib) + (double)E * SP_LN2;
        }
    }
    for (int off = 32; off >= 1; off >>= 1) err |= (uint32_t)__shfl_xor((int)err, off);
    if (lane == 0) {
        a.logp[rd] = err ? NAN : lmb;
        a.err[rd] = err;
    }
}

// first list entry of every read (and the total behind the last): the lists may live on the device only
static __global__ void __launch_bounds__(256) list_tables_entry_offsets(const uint64_t *read_off, const uint64_t *map_pos_off,
                                                                        uint64_t R, uint64_t *out) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r <= R) out[r] = map_pos_off[read_off[r]];
}

}  // namespace phmm
