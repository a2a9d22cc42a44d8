// Per-read transition usage over mapping lists (phmm_run_with_mapping_read_edges, include/phmm_amd_edges.h): the keyed,
// order-fixed segmented reduction of read_usage_kernel.h over the compacted records of the edge-term list pass
// (edge_list_records, mapping_flow.hip) instead of the states plane.
//
// The call holds n records, n < 2^31 - 1, in position order; record i carries the key the pass wrote (the edge id, or
// E + v for Begin -> v) and one value.
//   re_sort_keys     one thread per record: its position (binary search in the per-position record offsets), the read of
//                    that position (binary search in read_off) and its mapped key (the pass's key itself, or a gather
//                    through edge_key / init_key) -> (read << key_bits) | key, or RU_NO_KEY (all ones: sorts behind every
//                    read) for a term that is left out; the payload is i.
//   (stable radix sort of the pairs over the bits in use; ru_heads, an inclusive scan, ru_seg_starts and ru_row_off of
//   read_usage_kernel.h: the segments and the rows)
//   re_reduce        ru_reduce with one value per record: a wave takes 64 consecutive segments; a segment of at most
//                    RU_LANE_MAX records is summed by its lane in record order from 0, a longer one by the whole wave --
//                    lane l the records l, l + 64, ... in order from 0, then the butterfly of xor distance 32 .. 1.
//   re_col_sum       ru_col_sum with one value per row entry: one wave per key over its row entries in read order.
// No floating-point atomics anywhere; nothing depends on which wave runs first.
#pragma once

#include "read_usage_kernel.h"

namespace phmm {

// rec_off: [n_pos + 1] first record of every read position; read_off: [R + 1] first position of every read;
// edge_key [E] / init_key [N]: the mapped key or RU_NONE, null = that kind is left out; mapped == 0: the record's own key
static __global__ void __launch_bounds__(256) re_sort_keys(const uint64_t *rec_off, uint64_t n_pos, const uint64_t *read_off,
                                                           uint32_t R, const uint32_t *rec_key, uint32_t E, int mapped,
                                                           const uint32_t *edge_key, const uint32_t *init_key, uint32_t key_bits,
                                                           uint32_t n, uint64_t *keys, uint32_t *vals) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint64_t lo = 0, hi = n_pos;  // the last position p in [0, n_pos) with rec_off[p] <= i (empty ones are passed over)
    while (hi - lo > 1) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (rec_off[mid] <= i) lo = mid;
        else hi = mid;
    }
    const uint64_t p = lo;
    uint32_t rl = 0, rh = R;  // the last read r in [0, R) with read_off[r] <= p
    while (rh - rl > 1) {
        const uint32_t mid = rl + ((rh - rl) >> 1);
        if (read_off[mid] <= p) rl = mid;
        else rh = mid;
    }
    uint32_t k = rec_key[i];
    if (mapped) {
        const uint32_t *map = k < E ? edge_key : init_key;
        k = map ? map[k < E ? k : k - E] : RU_NONE;
    }
    keys[i] = k == RU_NONE ? RU_NO_KEY : ((uint64_t)rl << key_bits) | k;
    vals[i] = i;
}

// val: the records' values; S segments (the RU_NO_KEY one is not among them); out_keys / out_usage: the handle's arrays
static __global__ void __launch_bounds__(64 * RU_WAVES) re_reduce(const double *val, const uint64_t *keys, const uint32_t *vals,
                                                                  const uint32_t *seg_start, uint32_t S, uint32_t key_mask,
                                                                  uint32_t *out_keys, double *out_usage) {
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
        double sm = 0.0;
        for (uint32_t t = 0; t < len; t++) sm += val[vals[b + t]];
        out_usage[j] = sm;
    }
    uint64_t longs = __ballot(len > RU_LANE_MAX);
    while (longs) {
        const int src = __ffsll((long long)longs) - 1;
        longs &= longs - 1;
        const uint32_t lb = __shfl(b, src), ll = __shfl(len, src);
        double sm = 0.0;
        for (uint32_t t = lane; t < ll; t += 64) sm += val[vals[lb + t]];
        sm = ru_butterfly(sm);
        if (lane == 0) out_usage[base + src] = sm;
    }
}

// the column totals: sorted_keys / sorted_rows are the T row entries of all reads, stably sorted by key (so in read
// order within a key); usage is the handle's [T]; totals [K]
static __global__ void __launch_bounds__(64 * RU_WAVES) re_col_sum(const uint32_t *sorted_keys, const uint32_t *sorted_rows,
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
    double sm = 0.0;
    for (uint32_t t = lo + lane; t < e0; t += 64) sm += usage[sorted_rows[t]];
    sm = ru_butterfly(sm);
    if (lane == 0) totals[k] = sm;
}

}  // namespace phmm
