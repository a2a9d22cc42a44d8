// Alignment records (phmm_run_with_mapping_alignments, include/phmm_amd_align.h): the rows of a chunk's best or sampled
// paths, staged in the workspace by the parent's walk kernel, compacted into a CIGAR and a node walk per alignment.
//
// The work is a segmented run-length encoding over a variable number of events per base.  alignments_kernel<WRITE>: one
// wave64 per alignment (four to a block, no block-level synchronisation), tiles of 64 bases with lane = base.  A lane
// loads its row -- 16-byte loads at stride 4 and 8; the rows of a tile are contiguous --, looks up the node of every
// Match and Del and keeps its at most 8 events in registers.  A CIGAR run starts where an op differs from the previous
// event's op, a walk run where a step's node is not the previous step's node plus one.  Across lanes the previous op is
// the last op of the nearest preceding lane that has an event and the previous node the last step of the nearest
// preceding lane that has a step (a 64-bit ballot, the highest set bit below the lane, one __shfl); both are carried from
// tile to tile in wave-uniform registers together with "none yet".
//   WRITE = false  adds up the starts: the CIGAR words and walk runs of the alignment, one 64-bit count each.
//   WRITE = true   numbers the starts with a wave prefix sum and stores them at the offsets the host scanned from those
//                  counts.  A run is stored once, when it closes: inside a lane by the lane's next start, across lanes by
//                  the first start of the nearest following lane that has one (ballot, lowest set bit above the lane,
//                  __shfl); the last run of a tile stays open in wave-uniform registers until a later tile or the end of
//                  the alignment closes it, so a run may span any number of tiles.
// Plain vector stores, 64-bit offsets, no atomics.  A row entry that names a slot outside its list or a node outside the
// model ends its row (the parent call reports such a walk as an error of its own; nothing is read out of bounds here).
#pragma once

#include "phmm_internal.h"

namespace phmm {

static constexpr uint32_t AL_NONE = 0xffffffffu, AL_INS_BEGIN = 0xfffffffdu;  // PHMM_PATH_NONE, PHMM_PATH_INS_BEGIN
static constexpr uint32_t AL_NO_OP = 0xfu;
static constexpr int AL_WAVES = 4;  // alignments per block

struct AlignArgs {
    const uint8_t *emis;
    uint32_t n_nodes;
    const uint8_t *bases;
    const uint64_t *read_off;     // [R+1]
    const uint64_t *map_pos_off;  // [total_bases+1]
    const uint32_t *map_nodes;
    const uint32_t *rows;         // row of base g in plane s: rows[(s * plane_rows + g - row0) * stride]
    uint64_t row0, plane_rows;
    uint32_t stride;
    uint32_t r0, planes;          // first read of the chunk; S' = max(n_samples, 1)
    uint64_t n_aln;               // alignments of the chunk: local index (r - r0) * planes + s
    uint64_t *cnt_ops, *cnt_runs; // count: [n_aln]
    const uint64_t *op_off, *run_off;  // write: [n_aln + 1], offsets into the three arrays below
    uint32_t *ops, *run_node, *run_len;
};

// the open run a tile hands to the next (wave-uniform): its output slot within the alignment, the index of its first
// event or step, and for a CIGAR run its op
struct AlOpen {
    uint32_t slot, idx, tag;
    bool open;
};

__device__ __forceinline__ uint32_t al_excl_scan(uint32_t v, uint32_t &total) {
    const int lane = threadIdx.x & 63;
    uint32_t x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    total = __shfl(x, 63);
    return x - v;
}

// value of the nearest lane below this one whose `has` is set, `carry` if there is none; then carry = the value of the
// highest such lane of the wave (kept if there is none).  Called by all 64 lanes.
__device__ __forceinline__ uint32_t al_prev(bool has, uint32_t v, uint32_t &carry, bool &any_before, bool &carry_any) {
    const int lane = threadIdx.x & 63;
    const uint64_t mask = __ballot(has);
    const uint64_t below = mask & (((uint64_t)1 << lane) - 1);
    const uint32_t got = __shfl(v, below ? 63 - __clzll((long long)below) : lane);
    const uint32_t prev = below ? got : carry;
    any_before = below ? true : carry_any;
    if (mask) {  // (uniform)
        carry = __shfl(v, 63 - __clzll((long long)mask));
        carry_any = true;
    }
    return prev;
}

// Closes runs across the lanes of a tile.  A lane with starts (`has`) holds its first start's index and its last start
// (slot, idx, tag), still open.  store(slot, len, tag) is called for every run that closes here: a lane's last run where a
// following lane has a start, and the run handed over by the earlier tiles.  Called by all 64 lanes.
template <class Store>
__device__ __forceinline__ void al_close(bool has, uint32_t first_idx, uint32_t slot, uint32_t idx, uint32_t tag, AlOpen &carry,
                                         Store store) {
    const int lane = threadIdx.x & 63;
    const uint64_t mask = __ballot(has);
    if (!mask) return;  // (uniform)
    const uint64_t above = lane == 63 ? 0 : mask & ~((((uint64_t)1 << lane) << 1) - 1);
    const uint32_t next_idx = __shfl(first_idx, above ? __ffsll((long long)above) - 1 : lane);
    if (has && above) store(slot, next_idx - idx, tag);
    const int lo = __ffsll((long long)mask) - 1, hi = 63 - __clzll((long long)mask);
    const uint32_t lo_idx = __shfl(first_idx, lo);
    if (carry.open && lane == 0) store(carry.slot, lo_idx - carry.idx, carry.tag);
    carry.slot = __shfl(slot, hi);
    carry.idx = __shfl(idx, hi);
    carry.tag = __shfl(tag, hi);
    carry.open = true;
}

template <bool WRITE> __global__ void __launch_bounds__(64 * AL_WAVES) alignments_kernel(const AlignArgs a) {
    const int lane = threadIdx.x & 63;
    const uint64_t al = (uint64_t)blockIdx.x * AL_WAVES + (threadIdx.x >> 6);
    if (al >= a.n_aln) return;  // (a whole wave)
    const uint32_t rd = a.r0 + (uint32_t)(al / a.planes), s = (uint32_t)(al % a.planes);
    const uint64_t b0 = a.read_off[rd], len = a.read_off[rd + 1] - b0;
    const uint32_t stride = a.stride;
    const uint32_t *plane = a.rows + ((uint64_t)s * a.plane_rows + (b0 - a.row0)) * stride;

    // carried from tile to tile (wave-uniform)
    uint32_t c_op = AL_NO_OP, c_node = 0;
    bool c_any_ev = false, c_any_step = false;
    uint32_t n_ev = 0, n_step = 0, n_cig = 0, n_run = 0;  // events, steps, CIGAR words and walk runs so far
    AlOpen o_cig{0, 0, 0, false}, o_run{0, 0, 0, false};
    uint32_t *ops = nullptr, *run_node = nullptr, *run_len = nullptr;
    if (WRITE) {
        ops = a.ops + a.op_off[al];
        run_node = a.run_node + a.run_off[al];
        run_len = a.run_len + a.run_off[al];
    }

    for (uint64_t t0 = 0; t0 < len; t0 += 64) {
        const uint64_t p = t0 + lane;
        // ---- the lane's events: op (4 bits each) and node
        uint32_t ev_ops = 0, ev_node[8], ne = 0;
#pragma unroll
        for (int c = 0; c < 8; c++) ev_node[c] = 0;
        if (p < len) {
            uint32_t row[8];
#pragma unroll
            for (int c = 0; c < 8; c++) row[c] = AL_NONE;
            const uint32_t *rp = plane + p * stride;
            if (stride == 4) {
                const uint4 v = *reinterpret_cast<const uint4 *>(rp);
                row[0] = v.x, row[1] = v.y, row[2] = v.z, row[3] = v.w;
            } else if (stride == 8) {
                const uint4 v = *reinterpret_cast<const uint4 *>(rp), w = *reinterpret_cast<const uint4 *>(rp + 4);
                row[0] = v.x, row[1] = v.y, row[2] = v.z, row[3] = v.w;
                row[4] = w.x, row[5] = w.y, row[6] = w.z, row[7] = w.w;
            } else {
#pragma unroll
                for (int c = 0; c < 8; c++)
                    if ((uint32_t)c < stride) row[c] = rp[c];
            }
            const uint64_t e0 = a.map_pos_off[b0 + p];
            const uint32_t n = (uint32_t)(a.map_pos_off[b0 + p + 1] - e0);
            const uint8_t x = a.bases[b0 + p];
            bool alive = true;
#pragma unroll
            for (int c = 0; c < 8; c++) {
                const uint32_t code = row[c];
                if (!alive || code == AL_NONE) {
                    alive = false;
                    continue;
                }
                uint32_t op, nd = 0;
                if (c == 0 && code == AL_INS_BEGIN) {
                    op = PHMM_ALN_INS;
                } else {
                    const uint32_t slot = code >> 2, kind = code & 3u;
                    if (slot >= n || (c == 0 ? kind > 1u : kind != 2u)) {
                        alive = false;
                        continue;
                    }
                    nd = a.map_nodes[e0 + slot];
                    if (nd >= a.n_nodes) {
                        alive = false;
                        continue;
                    }
                    op = c > 0 ? PHMM_ALN_DEL : kind == 1u ? PHMM_ALN_INS : a.emis[nd] == x ? PHMM_ALN_EQ : PHMM_ALN_DIFF;
                }
                ev_ops |= op << (4 * c);
                ev_node[c] = nd;
                ne = c + 1;
            }
        }
        // ---- what the lane shows its successors: its last op and its last step
        uint32_t ns = 0, last_node = 0;
#pragma unroll
        for (int c = 0; c < 8; c++)
            if ((uint32_t)c < ne && ((ev_ops >> (4 * c)) & 0xfu) != PHMM_ALN_INS) {
                ns++;
                last_node = ev_node[c];
            }
        const uint32_t last_op = ne ? (ev_ops >> (4 * (ne - 1))) & 0xfu : AL_NO_OP;
        bool any_ev, any_step;
        uint32_t pop = al_prev(ne > 0, last_op, c_op, any_ev, c_any_ev);
        uint32_t pnode = al_prev(ns > 0, last_node, c_node, any_step, c_any_step);
        if (!any_ev) pop = AL_NO_OP;
        // ---- the lane's starts
        uint32_t cig_starts = 0, run_starts = 0;
        {
            uint32_t q = pop, qn = pnode;
            bool qs = any_step;
#pragma unroll
            for (int c = 0; c < 8; c++)
                if ((uint32_t)c < ne) {
                    const uint32_t op = (ev_ops >> (4 * c)) & 0xfu;
                    cig_starts += op != q;
                    q = op;
                    if (op != PHMM_ALN_INS) {
                        run_starts += !qs || ev_node[c] != qn + 1;
                        qn = ev_node[c];
                        qs = true;
                    }
                }
        }
        uint32_t t_ev, t_step, t_cig, t_run;
        const uint32_t ev0 = n_ev + al_excl_scan(ne, t_ev), st0 = n_step + al_excl_scan(ns, t_step);
        const uint32_t cig0 = n_cig + al_excl_scan(cig_starts, t_cig), run0 = n_run + al_excl_scan(run_starts, t_run);
        if (WRITE) {
            // ---- the lane's runs: every run but its last closes inside the lane
            uint32_t q = pop, qn = pnode;
            bool qs = any_step;
            uint32_t k_cig = 0, k_run = 0, k_step = 0;
            uint32_t f_cig = 0, l_cig = 0, l_op = 0, f_run = 0, l_run = 0;
#pragma unroll
            for (int c = 0; c < 8; c++)
                if ((uint32_t)c < ne) {
                    const uint32_t op = (ev_ops >> (4 * c)) & 0xfu;
                    if (op != q) {
                        if (k_cig) ops[cig0 + k_cig - 1] = ((ev0 + c - l_cig) << 4) | l_op;
                        else f_cig = ev0 + c;
                        l_cig = ev0 + c;
                        l_op = op;
                        k_cig++;
                    }
                    q = op;
                    if (op != PHMM_ALN_INS) {
                        if (!qs || ev_node[c] != qn + 1) {
                            if (k_run) run_len[run0 + k_run - 1] = st0 + k_step - l_run;
                            else f_run = st0 + k_step;
                            l_run = st0 + k_step;
                            run_node[run0 + k_run] = ev_node[c];
                            k_run++;
                        }
                        qn = ev_node[c];
                        qs = true;
                        k_step++;
                    }
                }
            al_close(cig_starts > 0, f_cig, cig0 + cig_starts - 1, l_cig, l_op, o_cig,
                     [&](uint32_t slot, uint32_t n, uint32_t op) { ops[slot] = (n << 4) | op; });
            al_close(run_starts > 0, f_run, run0 + run_starts - 1, l_run, 0u, o_run,
                     [&](uint32_t slot, uint32_t n, uint32_t) { run_len[slot] = n; });
        }
        n_ev += t_ev;
        n_step += t_step;
        n_cig += t_cig;
        n_run += t_run;
    }
    if (lane == 0) {
        if (WRITE) {
            if (o_cig.open) ops[o_cig.slot] = ((n_ev - o_cig.idx) << 4) | o_cig.tag;
            if (o_run.open) run_len[o_run.slot] = n_step - o_run.idx;
        } else {
            a.cnt_ops[al] = n_cig;
            a.cnt_runs[al] = n_run;
        }
    }
}

}  // namespace phmm
