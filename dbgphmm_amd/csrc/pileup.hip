// phmm_run_with_mapping_pileup (include/phmm_amd_pileup.h): per read and node, the posterior by state split by the read
// base there, and the per-node totals -- a pileup on the graph (kernels in pileup_kernel.h).
//
// Host flow.  api.cpp has the reads checked on the host (pileup_check_bases: a byte other than A C G T is refused before
// any device work).  Then the keyed reduction of read_usage.hip (run_with_mapping_keyed_usage) runs as it does for the
// read-usage call -- the states pass into the workspace plane, chunks of whole reads, the stable sort, the segments, the
// sums into the handle, the sort of the handle's keys -- with this call's two ends: pu_sort_keys builds the key 4 v + c
// from the node and the read base of the entry's position, and pu_node_totals sums the sorted row entries into the nine
// columns of every node.
#include "pileup_kernel.h"

namespace phmm {

void pileup_check_bases(const phmm_reads *reads) {
    for (uint64_t r = 0; r < reads->R; r++)
        for (uint64_t g = reads->off[r]; g < reads->off[r + 1]; g++) {
            const uint8_t x = reads->bases[g];
            if (x != 'A' && x != 'C' && x != 'G' && x != 'T')
                PHMM_THROW(PHMM_EINVAL, "read " + std::to_string(r) + ", position " + std::to_string(g - reads->off[r]) +
                                            ": byte " + std::to_string((unsigned)x) + " is none of A C G T");
        }
}

void run_with_mapping_pileup(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mp, double *out_lf,
                             double *out_node_pileup, phmm_read_usage *h) {
    const uint32_t N = m->N;
    KeyedUsage ku;
    ku.K = 4 * N;
    ku.totals_doubles = 9 * (size_t)N;
    ku.totals_name = "out_node_pileup";
    ku.sort_keys = [&](hipStream_t s, const uint64_t *ent, uint32_t r0, uint32_t r1, uint32_t key_bits, uint32_t n,
                       uint64_t *keys, uint32_t *vals) {
        hipLaunchKernelGGL(pu_sort_keys, dim3((n + 255) / 256), dim3(256), 0, s, ent, r0, r1, reads->d_off.as<uint64_t>(),
                           mp->d_pos_off.as<uint64_t>(), mp->d_nodes.as<uint32_t>(), reads->d_bases.as<uint8_t>(), key_bits, n,
                           keys, vals);
    };
    ku.totals = [&](hipStream_t s, const uint32_t *sorted_keys, const uint32_t *sorted_rows, uint32_t T, const double *usage,
                    double *totals) {
        hipLaunchKernelGGL(pu_node_totals, dim3((N + RU_WAVES - 1) / RU_WAVES), dim3(64 * RU_WAVES), 0, s, sorted_keys,
                           sorted_rows, T, usage, N, totals);
    };
    run_with_mapping_keyed_usage(m, reads, mp, ku, out_lf, out_node_pileup, h);
}

}  // namespace phmm
