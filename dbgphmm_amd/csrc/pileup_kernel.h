// Pileup over mapping lists (phmm_run_with_mapping_pileup, include/phmm_amd_pileup.h): the two ends of the keyed
// reduction of read_usage_kernel.h that depend on the read base.
//
//   pu_sort_keys     one thread per entry of the chunk: the read of the entry as ru_sort_keys finds it, then the position
//                    within the read -- the last g in [read_off[r], read_off[r + 1]) with pos_off[g] <= a, so empty lists
//                    before, between and behind are passed over -- and the base there -> (read << key_bits) | (4 v + c),
//                    c = 0 A, 1 C, 2 G, 3 T (the host has refused every other byte); the payload is i.
//   pu_node_totals   the per-node totals [N][9]: the handle's row entries stably sorted by key (so in read order within a
//                    key), one wave per node as ru_col_sum takes one per key.  Lanes 0..4 find the first entry of the
//                    keys 4 v .. 4 v + 4; then per read base c the Match and Ins values of key 4 v + c (columns c and
//                    4 + c) and the Del values of all four keys in sorted order (column 8): lane-strided partial sums, then
//                    the butterfly of xor distance 32 .. 1.
// No floating-point atomics; nothing depends on which wave runs first.
#pragma once

#include "read_usage_kernel.h"

namespace phmm {

__device__ __forceinline__ uint32_t pu_base_code(uint8_t x) { return x == 'A' ? 0u : x == 'C' ? 1u : x == 'G' ? 2u : 3u; }

// ent: [R + 1] first entry of every read; r0, r1: the reads of the chunk; read_off: [R + 1] first position of every read;
// pos_off: [positions + 1]; bases: [positions]
static __global__ void __launch_bounds__(256) pu_sort_keys(const uint64_t *ent, uint32_t r0, uint32_t r1, const uint64_t *read_off,
                                                           const uint64_t *pos_off, const uint32_t *nodes, const uint8_t *bases,
                                                           uint32_t key_bits, uint32_t n, uint64_t *keys, uint32_t *vals) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t a = ent[r0] + i;
    uint32_t lo = r0, hi = r1;  // the last read r in [r0, r1) with ent[r] <= a
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (ent[mid] <= a) lo = mid;
        else hi = mid;
    }
    uint64_t g = read_off[lo], ge = read_off[lo + 1];  // the last position g of the read with pos_off[g] <= a
    while (ge - g > 1) {
        const uint64_t mid = g + ((ge - g) >> 1);
        if (pos_off[mid] <= a) g = mid;
        else ge = mid;
    }
    keys[i] = ((uint64_t)(lo - r0) << key_bits) | (4u * nodes[a] + pu_base_code(bases[g]));
    vals[i] = i;
}

// sorted_keys / sorted_rows: the T row entries of all reads, stably sorted by key; usage: the handle's [T][3];
// totals: [N][9] = Match by base, Ins by base, Del
static __global__ void __launch_bounds__(64 * RU_WAVES) pu_node_totals(const uint32_t *sorted_keys, const uint32_t *sorted_rows,
                                                                       uint32_t T, const double *usage, uint32_t N,
                                                                       double *totals) {
    const uint32_t v = blockIdx.x * RU_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (v >= N) return;  // (a whole wave)
    // lane c = 0..4: the first index with key >= 4 v + c (64-bit: 4 v + 4 may be 2^32)
    const uint64_t want = 4ull * v + (uint32_t)(lane < 4 ? lane : 4);
    uint32_t lo = 0, hi = T;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (sorted_keys[mid] < want) lo = mid + 1;
        else hi = mid;
    }
    uint32_t b[5];
#pragma unroll
    for (int c = 0; c < 5; c++) b[c] = __shfl(lo, c);
    double *o = totals + 9 * (uint64_t)v;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        double sm = 0.0, si = 0.0;
        for (uint32_t t = b[c] + lane; t < b[c + 1]; t += 64) {
            const double *p = usage + 3 * (uint64_t)sorted_rows[t];
            sm += p[0];
            si += p[1];
        }
        sm = ru_butterfly(sm);
        si = ru_butterfly(si);
        if (lane == 0) {
            o[c] = sm;
            o[4 + c] = si;
        }
    }
    double sd = 0.0;
    for (uint32_t t = b[0] + lane; t < b[4]; t += 64) sd += usage[3 * (uint64_t)sorted_rows[t] + 2];
    sd = ru_butterfly(sd);
    if (lane == 0) o[8] = sd;
}

}  // namespace phmm
