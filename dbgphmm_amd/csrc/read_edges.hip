// phmm_run_with_mapping_read_edges (include/phmm_amd_edges.h): how often every read crossed every edge (or key of a
// caller's edge map) -- a sparse read-by-key matrix, CSR over the reads (kernels in read_edges_kernel.h).
//
// Host flow.  edge_list_records (mapping_flow.hip), the front half of phmm_run_with_mapping_edges, leaves the records of
// the edge-term list pass on the device, compacted in position order.  Where the summed call sorts them by key alone,
// this one keeps the read:
//   1. re_sort_keys: (read << key_bits) | mapped key per record, the record's index as payload;
//   2. a stable hipcub radix sort of the pairs over the bits in use;
//   3. ru_heads, an inclusive scan and ru_seg_starts: the segments; their count and the last key come back to the host
//      (the records that are left out form the last segment, which is dropped) and the handle's arrays are allocated;
//   4. ru_row_off and re_reduce write row_off, keys and usage straight into the handle.
// Then the column totals over all reads: the handle's keys, stably sorted with their row index, one wave per key
// (re_col_sum), and the two end-term scalars of every read on the host (edge_end_terms).
// The reduction is not chunked: its scratch (32 bytes per record and the sort's temporary storage, one workspace
// buffer) must fit the workspace limit beside nothing else, or the call refuses.  All workspace buffers go back when
// the call ends (EdgeScratchRelease); what the handle owns is its own.
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "read_edges_kernel.h"

namespace phmm {

namespace {

struct Carver {
    size_t top = 0;
    size_t take(size_t bytes) {
        top = (top + 255) / 256 * 256;
        const size_t o = top;
        top += bytes;
        return o;
    }
};

uint32_t bits_for(uint64_t n) {  // smallest b >= 1 with 2^b >= n
    uint32_t b = 1;
    while (b < 63 && (1ull << b) < n) b++;
    return b;
}

}  // namespace

void run_with_mapping_read_edges(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mp, uint32_t K, bool mapped,
                                 const uint32_t *edge_key, const uint32_t *init_key, double *out_lf, double *out_end_terms,
                                 double *out_key_usage, phmm_read_edges *h) {
    hipStream_t s = current_stream();
    const uint64_t R = reads->R, n_pos = reads->total;
    const uint32_t N = m->N, E = m->E;
    if (R >= (1ull << 31)) PHMM_THROW(PHMM_ECAPACITY, "more than 2^31 - 1 reads");
    EdgeScratchRelease release_scratch{m};
    EdgeRecords er;
    edge_list_records(m, reads, mp, er);  // (its refusals come before any write of this call)
    CallStats &st = stats();
    st.ms[2] = 0.0;  // index 2 counts the reduction alone; the other indices stay those of the list pass
    st.launches[2] = st.cells[2] = 0;
    if (er.total > (uint64_t)INT32_MAX - 1)
        PHMM_THROW(PHMM_ECAPACITY, "more than 2^31 - 2 edge records (call it on fewer reads)");
    const uint32_t n = (uint32_t)er.total;

    // the end terms: two scalars per read
    std::vector<double> end_terms(2 * R);
    if (out_end_terms) {
        std::vector<double> logib(std::max<uint64_t>(reads->max_len, 1));
        HIP_CHECK(hipMemcpy(logib.data(), er.logib, sizeof(double) * logib.size(), hipMemcpyDeviceToHost));
        for (uint64_t r = 0; r < R; r++) edge_end_terms(m, reads, er.lf, logib, r, end_terms[2 * r], end_terms[2 * r + 1]);
    }
    phmm_read_edges local;
    phmm_read_edges *u = h ? h : &local;
    if (h || out_key_usage) {
        LaunchTimer tm(timing_enabled());  // device time of the whole stage on its stream
        tm.begin();
        WorkSet &ws = m->wset();
        DevBuf &arena = ws.aux[20], &d_map = ws.aux[21], &d_totals = ws.aux[16];
        const uint32_t *dek = nullptr, *dik = nullptr;
        if (mapped) {
            d_map.reserve(sizeof(uint32_t) * ((size_t)E + N + 1));
            if (edge_key && E) {
                HIP_CHECK(hipMemcpyAsync(d_map.p, edge_key, sizeof(uint32_t) * E, hipMemcpyHostToDevice, s));
                dek = d_map.as<uint32_t>();
            }
            if (init_key) {
                HIP_CHECK(hipMemcpyAsync(d_map.as<uint32_t>() + E, init_key, sizeof(uint32_t) * N, hipMemcpyHostToDevice, s));
                dik = d_map.as<uint32_t>() + E;
            }
        }
        const uint32_t key_bits = bits_for((uint64_t)K + 1);  // (the all-ones key is left to RU_NO_KEY)
        const uint32_t key_mask = key_bits >= 32 ? 0xffffffffu : (1u << key_bits) - 1;
        u->R = R;
        u->K = K;
        u->device = m->pool->device;
        u->d_row_off.reserve(sizeof(uint64_t) * (R + 1));
        uint32_t S = 0;
        const uint64_t *sk = nullptr;
        const uint32_t *seg_start = nullptr;
        if (n) {
            const int end_bit = (int)(key_bits + bits_for(R));
            size_t sb = 0, cb = 0;
            HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, sb, (const uint64_t *)nullptr, (uint64_t *)nullptr,
                                                         (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)n, 0, end_bit,
                                                         s));
            HIP_CHECK(hipcub::DeviceScan::InclusiveSum(nullptr, cb, (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)n, s));
            const size_t tb = std::max(sb, cb);
            Carver c;
            const size_t o_k0 = c.take(sizeof(uint64_t) * n), o_k1 = c.take(sizeof(uint64_t) * n),
                         o_v0 = c.take(sizeof(uint32_t) * n), o_v1 = c.take(sizeof(uint32_t) * n),
                         o_seg = c.take(sizeof(uint32_t) * n), o_start = c.take(sizeof(uint32_t) * ((size_t)n + 1)),
                         o_tmp = c.take(tb);
            if (c.top > table_budget(*m->pool))
                PHMM_THROW(PHMM_ECAPACITY, "the reduction's scratch (32 bytes per edge record and the sort's) exceeds the "
                                           "workspace limit (call it on fewer reads)");
            arena.reserve(c.top);
            char *ap = arena.as<char>();
            uint64_t *k0 = (uint64_t *)(ap + o_k0), *k1 = (uint64_t *)(ap + o_k1);
            uint32_t *v0 = (uint32_t *)(ap + o_v0), *v1 = (uint32_t *)(ap + o_v1), *seg = (uint32_t *)(ap + o_seg),
                     *start = (uint32_t *)(ap + o_start);
            const dim3 grid((n + 255) / 256), block(256);
            hipLaunchKernelGGL(re_sort_keys, grid, block, 0, s, er.pos_off, n_pos, reads->d_off.as<uint64_t>(), (uint32_t)R,
                               er.key, E, mapped ? 1 : 0, dek, dik, key_bits, n, k0, v0);
            HIP_CHECK(hipGetLastError());
            sb = tb;
            HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(ap + o_tmp, sb, (const uint64_t *)k0, k1, (const uint32_t *)v0, v1,
                                                         (int)n, 0, end_bit, s));
            hipLaunchKernelGGL(ru_heads, grid, block, 0, s, (const uint64_t *)k1, n, seg);
            HIP_CHECK(hipGetLastError());
            sb = tb;
            HIP_CHECK(hipcub::DeviceScan::InclusiveSum(ap + o_tmp, sb, (const uint32_t *)seg, seg, (int)n, s));
            hipLaunchKernelGGL(ru_seg_starts, grid, block, 0, s, (const uint64_t *)k1, (const uint32_t *)seg, n, start);
            HIP_CHECK(hipGetLastError());
            uint32_t s_total = 0;
            uint64_t last_key = 0;
            HIP_CHECK(hipMemcpyAsync(&s_total, seg + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipMemcpyAsync(&last_key, k1 + (n - 1), sizeof(uint64_t), hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipStreamSynchronize(s));
            st.launches[2] += 5;
            S = s_total - (last_key == RU_NO_KEY ? 1u : 0u);
            sk = k1;
            seg_start = start;
            trace("read edges segments");
            u->d_keys.reserve(sizeof(uint32_t) * std::max<uint32_t>(S, 1));
            u->d_usage.reserve(sizeof(double) * std::max<uint32_t>(S, 1));
            if (S) {
                hipLaunchKernelGGL(re_reduce, dim3((S + 64 * RU_WAVES - 1) / (64 * RU_WAVES)), dim3(64 * RU_WAVES), 0, s, er.val,
                                   sk, (const uint32_t *)v1, seg_start, S, key_mask, u->d_keys.as<uint32_t>(),
                                   u->d_usage.as<double>());
                HIP_CHECK(hipGetLastError());
                st.launches[2]++;
            }
        }
        hipLaunchKernelGGL(ru_row_off, dim3((unsigned)((R + 256) / 256)), dim3(256), 0, s, sk, seg_start, S, 0u, (uint32_t)R,
                           key_bits, (uint64_t)0, u->d_row_off.as<uint64_t>());
        HIP_CHECK(hipGetLastError());
        st.launches[2]++;
        HIP_CHECK(hipStreamSynchronize(s));  // the arena is the totals' next
        u->total = S;
        trace("read edges rows");

        // column totals: the row entries of all reads, stably sorted by key, one wave per key
        if (out_key_usage) {
            const uint32_t T = S;
            size_t tb = 0;
            if (T)
                HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                                             (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)T, 0,
                                                             (int)key_bits, s));
            Carver c;
            const size_t o_k1 = c.take(sizeof(uint32_t) * T), o_v0 = c.take(sizeof(uint32_t) * T),
                         o_v1 = c.take(sizeof(uint32_t) * T), o_tmp = c.take(tb);
            arena.reserve(std::max<size_t>(c.top, 256));
            d_totals.reserve(sizeof(double) * std::max<uint32_t>(K, 1));
            char *ap = arena.as<char>();
            uint32_t *k1 = (uint32_t *)(ap + o_k1), *v0 = (uint32_t *)(ap + o_v0), *v1 = (uint32_t *)(ap + o_v1);
            if (T) {
                hipLaunchKernelGGL(ru_iota, dim3((T + 255) / 256), dim3(256), 0, s, T, v0);
                HIP_CHECK(hipGetLastError());
                HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(ap + o_tmp, tb, (const uint32_t *)u->d_keys.as<uint32_t>(), k1,
                                                             (const uint32_t *)v0, v1, (int)T, 0, (int)key_bits, s));
                st.launches[2] += 2;
            }
            if (K) {
                hipLaunchKernelGGL(re_col_sum, dim3((K + RU_WAVES - 1) / RU_WAVES), dim3(64 * RU_WAVES), 0, s,
                                   (const uint32_t *)k1, (const uint32_t *)v1, T, (const double *)u->d_usage.as<double>(), K,
                                   d_totals.as<double>());
                HIP_CHECK(hipGetLastError());
                st.launches[2]++;
            }
            trace("read edges totals");
        }
        tm.end();
        st.ms[2] += tm.total_ms();
        st.cells[2] = n;
        if (out_key_usage && K) copy_out(out_key_usage, d_totals.p, sizeof(double) * K);
    }
    put_doubles(out_end_terms, end_terms.data(), 2 * R);
    put_doubles(out_lf, er.lf.data(), R);
    HIP_CHECK(hipStreamSynchronize(s));
    trace("read edges outputs");
}

void read_edges_export(const phmm_read_edges *u, uint64_t *row_off, uint32_t *keys, double *usage) {
    if (u->R == 0) {  // (a call without reads: nothing on the device)
        const uint64_t zero = 0;
        put_bytes(row_off, &zero, sizeof zero);
        return;
    }
    copy_out(row_off, u->d_row_off.p, sizeof(uint64_t) * (u->R + 1));
    copy_out(keys, u->d_keys.p, sizeof(uint32_t) * u->total);
    copy_out(usage, u->d_usage.p, sizeof(double) * u->total);
}

}  // namespace phmm
