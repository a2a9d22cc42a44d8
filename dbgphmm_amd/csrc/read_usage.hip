// phmm_run_with_mapping_read_usage (include/phmm_amd_usage.h): how often every read used every node (or node group), by
// state -- a sparse read-by-key matrix, CSR over the reads (kernels in read_usage_kernel.h).
//
// Host flow.  run_with_mapping_states writes its per-entry values into a workspace plane (24 bytes per list entry, the
// whole call), as the MEA call does; nothing of it leaves the device.  The reads are then cut into chunks of consecutive
// whole reads of at most 2^30 list entries whose scratch fits the workspace budget (phmm_set_workspace_limit;
// table_budget otherwise), one read at the least.  Per chunk:
//   1. ru_sort_keys: (read << key_bits) | key per entry, the entry's index as payload;
//   2. a stable hipcub radix sort of the pairs over the bits in use;
//   3. ru_heads, an inclusive scan and ru_seg_starts: the segments; their count and the last key come back to the host
//      (the entries of nodes in no group form the last segment, which is dropped) and the handle's arrays grow to hold
//      the chunk's rows (a device copy keeps the earlier chunks'; a call of one chunk allocates each array once);
//   4. ru_row_off and ru_reduce write row_off, keys and usage straight into the handle.
// Then the column totals over all reads: the handle's keys, stably sorted with their row index, one wave per key
// (ru_col_sum).  That sort is not chunked.
// All scratch is carved from one workspace buffer (aux[1]); what the handle owns is its own.
//
// The flow is run_with_mapping_keyed_usage; what a key is comes in through KeyedUsage (phmm_internal.h): the builder of the
// sort keys in step 1 and the kernel behind the totals.  This call passes ru_sort_keys and ru_col_sum, the pileup call
// (pileup.hip) its own two.
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "read_usage_kernel.h"

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

// temporary storage of the chunk's sort and scan at n entries
size_t chunk_temp_bytes(uint32_t n, int end_bit, hipStream_t s) {
    size_t sb = 0, cb = 0;
    HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, sb, (const uint64_t *)nullptr, (uint64_t *)nullptr,
                                                 (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)n, 0, end_bit, s));
    HIP_CHECK(hipcub::DeviceScan::InclusiveSum(nullptr, cb, (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)n, s));
    return std::max(sb, cb);
}

// the chunk's own arrays: sort keys in and out (8 + 8), payloads in and out (4 + 4), segment of the entry (4), segment
// starts (4): 32 bytes per entry
uint64_t chunk_bytes(uint64_t n, size_t temp) { return 32 * n + temp + 8 * 256; }

}  // namespace

void run_with_mapping_keyed_usage(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mp, const KeyedUsage &ku,
                                  double *out_lf, double *out_key_usage, phmm_read_usage *h) {
    hipStream_t s = current_stream();
    const uint32_t K = ku.K;
    if (m->dev.max_degree > 8) PHMM_THROW(PHMM_EINVAL, "sparse path supports node degree <= 8 (MultiDbg MAX_DEGREE is 5)");
    const uint64_t R = reads->R, n_ent = mp->total_entries, plane = sizeof(double) * 3 * n_ent;
    for (uint64_t r = 0; r < R; r++)
        if (mp->read_max_list[r] > (uint32_t)PHMM_MAX_ACTIVE_NODES)
            PHMM_THROW(PHMM_ECAPACITY, "a mapping position lists more than 400 nodes");
    if (R >= RU_NONE) PHMM_THROW(PHMM_ECAPACITY, "more than 2^32 - 2 reads");
    if (plane > table_budget(*m->pool))
        PHMM_THROW(PHMM_ECAPACITY, "the states plane (24 bytes per list entry) exceeds the workspace limit");
    WorkSet &ws = m->wset();
    DevBuf &d_w = ws.aux[0], &arena = ws.aux[1], &d_ent = ws.aux[3];
    d_w.reserve(std::max<uint64_t>(plane, 8));
    // the posteriors by state, written in place on the device (its refusals come before any of its writes)
    std::vector<double> lf(R);
    run_with_mapping_states(m, reads, mp, lf.data(), n_ent ? d_w.as<double>() : nullptr, nullptr);
    CallStats &st = stats();
    st.ms[2] = 0.0;  // index 2 counts this stage alone; the other indices stay those of the states pass
    st.launches[2] = st.cells[2] = 0;
    phmm_read_usage local;
    phmm_read_usage *u = h ? h : &local;
    if (!h && !out_key_usage) {
        put_doubles(out_lf, lf.data(), R);
        return;
    }
    LaunchTimer tm(timing_enabled());  // device time of the whole stage on its stream
    tm.begin();
    upload_reads(reads);
    upload_mappings(mp);
    if (ku.setup) ku.setup();
    const uint32_t key_bits = bits_for((uint64_t)K + 1);  // (the all-ones key is left to RU_NO_KEY)
    const uint32_t key_mask = key_bits >= 32 ? 0xffffffffu : (1u << key_bits) - 1;

    // first entry of every read: the lists may live on the device only
    std::vector<uint64_t> ent(R + 1);
    d_ent.reserve(sizeof(uint64_t) * (R + 1));
    hipLaunchKernelGGL(ru_entry_offsets, dim3((unsigned)((R + 256) / 256)), dim3(256), 0, s, reads->d_off.as<uint64_t>(),
                       mp->d_pos_off.as<uint64_t>(), R, d_ent.as<uint64_t>());
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(ent.data(), d_ent.p, sizeof(uint64_t) * (R + 1), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    st.launches[2]++;

    // the most entries a chunk may hold: hipcub counts in int, and the chunk's scratch fits the budget
    const uint64_t fixed = plane + sizeof(uint64_t) * (R + 1) + ku.fixed_bytes;
    const uint64_t limit = table_budget(*m->pool), budget = limit > fixed ? limit - fixed : 0;
    uint64_t cap = std::min<uint64_t>(std::max<uint64_t>(n_ent, 1), 1ull << 30);
    while (cap > 1 && chunk_bytes(cap, chunk_temp_bytes((uint32_t)cap, 64, s)) > budget) cap -= (cap + 3) / 4;

    u->R = R;
    u->K = K;
    u->device = m->pool->device;
    u->d_row_off.reserve(sizeof(uint64_t) * (R + 1));
    uint64_t rows_done = 0;
    trace("read usage setup");
    for (uint64_t r0 = 0; r0 < R;) {
        uint64_t r1 = r0 + 1;
        while (r1 < R && ent[r1 + 1] - ent[r0] <= cap) r1++;
        const uint64_t n64 = ent[r1] - ent[r0];
        if (n64 > (1ull << 30)) PHMM_THROW(PHMM_ECAPACITY, "a read has more than 2^30 list entries");
        const uint32_t n = (uint32_t)n64, nr = (uint32_t)(r1 - r0);
        uint32_t S = 0;
        const uint64_t *sk = nullptr;
        const uint32_t *seg_start = nullptr;
        if (n) {
            const int end_bit = (int)(key_bits + bits_for(nr));
            const size_t tb = chunk_temp_bytes(n, end_bit, s);
            Carver c;
            const size_t o_k0 = c.take(sizeof(uint64_t) * n), o_k1 = c.take(sizeof(uint64_t) * n),
                         o_v0 = c.take(sizeof(uint32_t) * n), o_v1 = c.take(sizeof(uint32_t) * n),
                         o_seg = c.take(sizeof(uint32_t) * n), o_start = c.take(sizeof(uint32_t) * ((size_t)n + 1)),
                         o_tmp = c.take(tb);
            arena.reserve(c.top);
            char *ap = arena.as<char>();
            uint64_t *k0 = (uint64_t *)(ap + o_k0), *k1 = (uint64_t *)(ap + o_k1);
            uint32_t *v0 = (uint32_t *)(ap + o_v0), *v1 = (uint32_t *)(ap + o_v1), *seg = (uint32_t *)(ap + o_seg),
                     *start = (uint32_t *)(ap + o_start);
            const dim3 grid((n + 255) / 256), block(256);
            ku.sort_keys(s, d_ent.as<uint64_t>(), (uint32_t)r0, (uint32_t)r1, key_bits, n, k0, v0);
            HIP_CHECK(hipGetLastError());
            size_t sb = tb;
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
            trace("read usage segments");
            grow_keep(u->d_keys, sizeof(uint32_t) * rows_done, sizeof(uint32_t) * (rows_done + S), s);
            grow_keep(u->d_usage, sizeof(double) * 3 * rows_done, sizeof(double) * 3 * (rows_done + S), s);
            if (S) {
                hipLaunchKernelGGL(ru_reduce, dim3((S + 64 * RU_WAVES - 1) / (64 * RU_WAVES)), dim3(64 * RU_WAVES), 0, s,
                                   d_w.as<double>(), ent[r0], sk, (const uint32_t *)v1, seg_start, S, key_mask,
                                   u->d_keys.as<uint32_t>() + rows_done, u->d_usage.as<double>() + 3 * rows_done);
                HIP_CHECK(hipGetLastError());
                st.launches[2]++;
            }
        }
        hipLaunchKernelGGL(ru_row_off, dim3((nr + 256) / 256), dim3(256), 0, s, sk, seg_start, S, (uint32_t)r0, (uint32_t)r1,
                           key_bits, rows_done, u->d_row_off.as<uint64_t>());
        HIP_CHECK(hipGetLastError());
        st.launches[2]++;
        HIP_CHECK(hipStreamSynchronize(s));  // the arena is the next chunk's
        trace("read usage rows");
        rows_done += S;
        r0 = r1;
    }
    u->total = rows_done;

    // column totals: the row entries of all reads, stably sorted by key, one wave per key
    double *d_tot = nullptr;
    if (out_key_usage) {
        if (rows_done > (uint64_t)INT32_MAX - 1)
            PHMM_THROW(PHMM_ECAPACITY, std::string(ku.totals_name) + ": more than 2^31 - 2 row entries (call it on fewer reads)");
        const uint32_t T = (uint32_t)rows_done;
        size_t tb = 0;
        if (T)
            HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                                         (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)T, 0,
                                                         (int)key_bits, s));
        Carver c;
        const size_t o_k1 = c.take(sizeof(uint32_t) * T), o_v0 = c.take(sizeof(uint32_t) * T),
                     o_v1 = c.take(sizeof(uint32_t) * T), o_tot = c.take(sizeof(double) * ku.totals_doubles), o_tmp = c.take(tb);
        arena.reserve(c.top);
        char *ap = arena.as<char>();
        uint32_t *k1 = (uint32_t *)(ap + o_k1), *v0 = (uint32_t *)(ap + o_v0), *v1 = (uint32_t *)(ap + o_v1);
        d_tot = (double *)(ap + o_tot);
        if (T) {
            hipLaunchKernelGGL(ru_iota, dim3((T + 255) / 256), dim3(256), 0, s, T, v0);
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(ap + o_tmp, tb, (const uint32_t *)u->d_keys.as<uint32_t>(), k1,
                                                         (const uint32_t *)v0, v1, (int)T, 0, (int)key_bits, s));
            st.launches[2] += 2;
        }
        ku.totals(s, (const uint32_t *)k1, (const uint32_t *)v1, T, (const double *)u->d_usage.as<double>(), d_tot);
        HIP_CHECK(hipGetLastError());
        st.launches[2]++;
        trace("read usage totals");
    }
    tm.end();
    st.ms[2] += tm.total_ms();
    st.cells[2] = n_ent;
    if (out_key_usage) copy_out(out_key_usage, d_tot, sizeof(double) * ku.totals_doubles);
    put_doubles(out_lf, lf.data(), R);
    HIP_CHECK(hipStreamSynchronize(s));
    trace("read usage outputs");
}

void run_with_mapping_read_usage(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mp, uint32_t K,
                                 const uint32_t *key_of, double *out_lf, double *out_key_usage, phmm_read_usage *h) {
    DevBuf &d_key_of = m->wset().aux[7];
    const uint32_t N = m->N;
    KeyedUsage ku;
    ku.K = K;
    ku.fixed_bytes = key_of ? sizeof(uint32_t) * N : 0;
    ku.totals_doubles = 3 * (size_t)K;
    ku.totals_name = "out_key_usage";
    ku.setup = [&] {
        if (key_of) d_key_of.upload(key_of, sizeof(uint32_t) * N);
    };
    ku.sort_keys = [&](hipStream_t s, const uint64_t *ent, uint32_t r0, uint32_t r1, uint32_t key_bits, uint32_t n,
                       uint64_t *keys, uint32_t *vals) {
        hipLaunchKernelGGL(ru_sort_keys, dim3((n + 255) / 256), dim3(256), 0, s, ent, r0, r1, mp->d_nodes.as<uint32_t>(),
                           key_of ? d_key_of.as<uint32_t>() : nullptr, key_bits, n, keys, vals);
    };
    ku.totals = [&](hipStream_t s, const uint32_t *sorted_keys, const uint32_t *sorted_rows, uint32_t T, const double *usage,
                    double *totals) {
        hipLaunchKernelGGL(ru_col_sum, dim3((K + RU_WAVES - 1) / RU_WAVES), dim3(64 * RU_WAVES), 0, s, sorted_keys,
                           sorted_rows, T, usage, K, totals);
    };
    run_with_mapping_keyed_usage(m, reads, mp, ku, out_lf, out_key_usage, h);
}

void read_usage_export(const phmm_read_usage *u, uint64_t *row_off, uint32_t *keys, double *usage) {
    if (u->R == 0) {  // (a call without reads: nothing on the device)
        const uint64_t zero = 0;
        put_bytes(row_off, &zero, sizeof zero);
        return;
    }
    copy_out(row_off, u->d_row_off.p, sizeof(uint64_t) * (u->R + 1));
    copy_out(keys, u->d_keys.p, sizeof(uint32_t) * u->total);
    copy_out(usage, u->d_usage.p, sizeof(double) * 3 * u->total);
}

}  // namespace phmm
