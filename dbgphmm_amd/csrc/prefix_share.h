// Prefix sharing of the dense head ("Prefix sharing"): column j of a read's dense forward table is
// a function of the model and of the bases x_0 .. x_j alone, so the first J columns are computed once per distinct
// prefix on 4^J virtual reads and every read of the plan takes them from there.  The planner's choice of J and the
// lane indexing.  No HIP types: sparse_dyn.hip, bwd_step (dense.hip) and the stand-alone program of
// tests/test_prefix_share_cpu.py share these functions.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define PHMM_SHARE_FN __host__ __device__ inline
#else
#define PHMM_SHARE_FN inline
#endif

namespace phmm {

static constexpr int SHARE_MIN_J = 2, SHARE_MAX_J = 6;
static constexpr int SHARE_W = 64;  // read-group width of the virtual plan and of the plans that share
// The virtual tables take at most 1 / SHARE_MEM_DIV of the main plan's table budget (limit_main, sparse_dyn.hip).
static constexpr uint64_t SHARE_MEM_DIV = 16;

// virtual reads of a J-base prefix, and the groups of 64 they fill
PHMM_SHARE_FN uint32_t share_lanes(int J) { return 1u << (2 * J); }
PHMM_SHARE_FN uint32_t share_groups(int J) { return (share_lanes(J) + SHARE_W - 1) / SHARE_W; }
// forward tables of the virtual plan: J kept columns of m, i, d
PHMM_SHARE_FN uint64_t share_table_bytes(int J, uint64_t N) {
    return (uint64_t)share_groups(J) * (uint64_t)J * N * SHARE_W * 24;
}

// group-columns saved by sharing J columns among ng read groups: ng J removed, J ceil(4^J / 64) added
PHMM_SHARE_FN int64_t share_gain(int ng, int J) { return (int64_t)ng * J - (int64_t)J * (int64_t)share_groups(J); }

// The planner's J for a plan of ng read groups on a model of N nodes: the J in 2..6 with the largest gain (the
// smallest such J on a tie) whose virtual tables fit `cap` bytes; 0 (off) when no J has a positive gain or none fits.
PHMM_SHARE_FN int share_choose_j(int ng, uint64_t N, uint64_t cap) {
    int best = 0;
    int64_t best_gain = 0;
    for (int J = SHARE_MIN_J; J <= SHARE_MAX_J; J++) {
        if (share_table_bytes(J, N) > cap) break;  // (the bytes grow with J)
        const int64_t g = share_gain(ng, J);
        if (g > best_gain) {
            best = J;
            best_gain = g;
        }
    }
    return best;
}

// The virtual lane of a prefix counts the first base as the least significant digit: idx = sum_i code(x_i) 4^i.
// digit[i] in 0..3.
PHMM_SHARE_FN uint32_t share_prefix_index(const uint8_t *digit, int J) {
    uint32_t idx = 0;
    for (int i = 0; i < J; i++) idx |= (uint32_t)(digit[i] & 3u) << (2 * i);
    return idx;
}
// digit i of a virtual lane = the code of its base at position i
PHMM_SHARE_FN uint32_t share_digit(uint32_t idx, int i) { return (idx >> (2 * i)) & 3u; }
// The virtual lane that stands for column j of a read with prefix index idx: idx mod 4^(j+1), the lane whose first
// j + 1 bases are the read's and whose other bases are code 0.  For j <= 2 it lies in virtual group 0.
PHMM_SHARE_FN uint32_t share_lane_of_column(uint32_t idx, int j) { return idx & (share_lanes(j + 1) - 1u); }

}  // namespace phmm
