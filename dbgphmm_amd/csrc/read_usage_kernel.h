// Per-read node usage over mapping lists (phmm_run_with_mapping_read_usage, include/phmm_amd_usage.h): the keyed,
// order-fixed segmented reduction over the plane the states pass leaves on the device.
//
// A chunk of whole reads holds n list entries, n < 2^31, entry a = ent0 + i.
//   ru_sort_keys     one thread per entry: the read of the entry (binary search in the reads' first-entry offsets) and
//                    the key of its node -> (read << key_bits) | key, or RU_NO_KEY (all ones: sorts behind every read)
//                    for a node in no group; the payload is i.
//   (stable radix sort of the pairs over the bits in use)
//   ru_heads         head[i] = 1 where the sorted key differs from the one before it.  An inclusive scan turns the flags
//                    into 1 + the segment of every entry; ru_seg_starts scatters the first entry of every segment.
//   ru_row_off       one thread per read of the chunk: the first segment of a read >= r (binary search): the handle's
//                    row_off.
//   ru_reduce        the sums.  A wave takes 64 consecutive segments.  A segment of at most RU_LANE_MAX entries is summed
//                    by its lane, alone, in entry order (the sort is stable, so sorted order within a segment IS entry
//                    order), starting from 0.  A longer segment is summed by the whole wave: lane l the entries l, l + 64,
//                    ... in order from 0, then the 64 partial sums in a butterfly of xor distance 32, 16, 8, 4, 2, 1.
//                    Which of the two a segment gets depends on its length alone, so a sum is a function of the segment's
//                    terms in their order and of nothing else.  Every term is exp of the plane's value, 0 for -inf.
//   ru_col_sum       the column totals: the row entries of all reads, stably sorted by key, one wave per key as
//                    map_node_freq (mapping_flow.hip) does it -- lane-strided partial sums in read order, then the
//                    butterfly above.
// No floating-point atomics anywhere; nothing depends on which wave runs first.
// The kernels have internal linkage: read_edges_kernel.h uses ru_heads, ru_seg_starts, ru_row_off and ru_iota from a
// second translation unit.
#pragma once

#include "phmm_internal.h"

namespace phmm {

static constexpr uint64_t RU_NO_KEY = ~0ull;
static constexpr uint32_t RU_NONE = 0xffffffffu;
static constexpr uint32_t RU_LANE_MAX = 64;  // longest segment a single lane sums
static constexpr int RU_WAVES = 4;           // waves per block of the two reduction kernels

// first entry of every read: ent[r] = pos_off[read_off[r]], r = 0..R
static __global__ void __launch_bounds__(256) ru_entry_offsets(const uint64_t *read_off, const uint64_t *pos_off, uint64_t R,
                                                               uint64_t *ent) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r <= R) ent[r] = pos_off[read_off[r]];
}

// ent: the offsets above; r0, r1: the reads of the chunk; key_of: [N] group of the node or RU_NONE, null = the node itself
static __global__ void __launch_bounds__(256) ru_sort_keys(const uint64_t *ent, uint32_t r0, uint32_t r1, const uint32_t *nodes,
                                                           const uint32_t *key_of, uint32_t key_bits, uint32_t n, uint64_t *keys,
                                                           uint32_t *vals) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t a = ent[r0] + i;
    uint32_t lo = r0, hi = r1;  // the last read r in [r0, r1) with ent[r] <= a (empty reads before it are passed over)
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (ent[mid] <= a) lo = mid;
        else hi = mid;
    }
    const uint32_t v = nodes[a], k = key_of ? key_of[v] : v;
    keys[i] = k == RU_NONE ? RU_NO_KEY : ((uint64_t)(lo - r0) << key_bits) | k;
    vals[i] = i;
}

static __global__ void __launch_bounds__(256) ru_heads(const uint64_t *keys, uint32_t n, uint32_t *head) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) head[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}

// seg_incl: the inclusive scan of the heads; seg_start[S] = n closes the last segment
static __global__ void __launch_bounds__(256) ru_seg_starts(const uint64_t *keys, const uint32_t *seg_incl, uint32_t n,
                                                            uint32_t *seg_start) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (i == 0 || keys[i] != keys[i - 1]) seg_start[seg_incl[i] - 1] = i;
    if (i == n - 1) seg_start[seg_incl[i]] = n;
}

// row_off[r] = rows_done + the first of the chunk's S segments whose read is >= r - r0, for r = r0 .. r1 (r1 gets
// rows_done + S: the next chunk overwrites it with the same value)
static __global__ void __launch_bounds__(256) ru_row_off(const uint64_t *keys, const uint32_t *seg_start, uint32_t S, uint32_t r0,
                                                         uint32_t r1, uint32_t key_bits, uint64_t rows_done, uint64_t *row_off) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j > r1 - r0) return;
    uint32_t lo = 0, hi = S;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((keys[seg_start[mid]] >> key_bits) < j) lo = mid + 1;
        else hi = mid;
    }
    row_off[r0 + j] = rows_done + lo;
}

__device__ __forceinline__ double ru_exp(double l) { return l > -INFINITY ? exp(l) : 0.0; }

__device__ __forceinline__ double ru_butterfly(double v) {
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// plane: [total_entries][3] logs; ent0: the first entry of the chunk; S segments (the RU_NO_KEY one is not among them)
// out_keys / out_usage: the handle's arrays at the chunk's first row entry
static __global__ void __launch_bounds__(64 * RU_WAVES) ru_reduce(const double *plane, uint64_t ent0, const uint64_t *keys,
                                                                  const uint32_t *vals, const uint32_t *seg_start, uint32_t S,
                                                                  uint32_t key_mask, uint32_t *out_keys, double *out_usage) {
    const int lane = threadIdx.x & 63;
    const uint32_t base = (blockIdx.x * RU_WAVES + (threadIdx.x >> 6)) * 64;
    if (base >= S) return;  // (a whole wave)
    const uint32_t j = base + lane;
    uint32_t b = 0, len = 0;
    if (j < S) {
        b = seg_start[j];
        len = seg_start[j + 1] - b;
        out_keys[j] = (uint32_t)keys[b] & key_mask;
    }
    if (len && len <= RU_LANE_MAX) {
        double sm = 0.0, si = 0.0, sd = 0.0;
        for (uint32_t t = 0; t < len; t++) {
            const double *p = plane + 3 * (ent0 + vals[b + t]);
            sm += ru_exp(p[0]);
            si += ru_exp(p[1]);
            sd += ru_exp(p[2]);
        }
        double *o = out_usage + 3 * (uint64_t)j;
        o[0] = sm;
        o[1] = si;
        o[2] = sd;
    }
    uint64_t longs = __ballot(len > RU_LANE_MAX);
    while (longs) {
        const int src = __ffsll((long long)longs) - 1;
        longs &= longs - 1;
        const uint32_t lb = __shfl(b, src), ll = __shfl(len, src);
        double sm = 0.0, si = 0.0, sd = 0.0;
        for (uint32_t t = lane; t < ll; t += 64) {
            const double *p = plane + 3 * (ent0 + vals[lb + t]);
            sm += ru_exp(p[0]);
            si += ru_exp(p[1]);
            sd += ru_exp(p[2]);
        }
        sm = ru_butterfly(sm);
        si = ru_butterfly(si);
        sd = ru_butterfly(sd);
        if (lane == 0) {
            double *o = out_usage + 3 * (uint64_t)(base + src);
            o[0] = sm;
            o[1] = si;
            o[2] = sd;
        }
    }
}

// the column totals: sorted_keys / sorted_rows are the T row entries of all reads, stably sorted by key (so in read
// order within a key); usage is the handle's [T][3]; totals [K][3]
static __global__ void __launch_bounds__(64 * RU_WAVES) ru_col_sum(const uint32_t *sorted_keys, const uint32_t *sorted_rows,
                                                                   uint32_t T, const double *usage, uint32_t K, double *totals) {
    const uint32_t k = blockIdx.x * RU_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (k >= K) return;  // (a whole wave)
    uint32_t lo = 0, hi = T;
    while (lo < hi) {  // first index with key >= k
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (sorted_keys[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    uint32_t e0 = lo, e1 = T;
    while (e0 < e1) {  // first index with key > k
        const uint32_t mid = e0 + ((e1 - e0) >> 1);
        if (sorted_keys[mid] <= k) e0 = mid + 1;
        else e1 = mid;
    }
    double sm = 0.0, si = 0.0, sd = 0.0;
    for (uint32_t t = lo + lane; t < e0; t += 64) {
        const double *p = usage + 3 * (uint64_t)sorted_rows[t];
        sm += p[0];
        si += p[1];
        sd += p[2];
    }
    sm = ru_butterfly(sm);
    si = ru_butterfly(si);
    sd = ru_butterfly(sd);
    if (lane == 0) {
        totals[3 * (uint64_t)k] = sm;
        totals[3 * (uint64_t)k + 1] = si;
        totals[3 * (uint64_t)k + 2] = sd;
    }
}

static __global__ void __launch_bounds__(256) ru_iota(uint32_t n, uint32_t *v) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) v[i] = i;
}

}  // namespace phmm
