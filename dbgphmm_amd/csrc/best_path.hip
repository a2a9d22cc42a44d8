// phmm_run_with_mapping_best_path: the max-product pass over mapping lists and its traceback (best_path_kernel.h).
//
// Host flow.  The reads are cut into chunks of consecutive reads whose back-pointer records (16 bytes per list entry)
// and, for a host out_path, staged rows fit the workspace budget (phmm_set_workspace_limit; table_budget otherwise).
// Per chunk: the forward kernel of the <= 64 class and of the 400 class over the chunk's reads, then the traceback
// over all of them, then the rows of a host out_path go out -- or, with a RowSink (alignments.hip), the staged rows are
// handed to it on the device.  ln P and the counts of all reads stay in the workspace until the last chunk is done.
// A read's results depend on the read and its lists alone, so the chunking shows nowhere.
#include <algorithm>
#include <cstring>

#include "best_path_kernel.h"

namespace phmm {

namespace {

bool is_device_pointer(const void *p) {
    hipPointerAttribute_t at;
    const bool dev = hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeDevice;
    if (!dev) (void)hipGetLastError();
    return dev;
}

struct CallTimer {  // device time of the whole call on its stream (index 2 of phmm_last_call_stats)
    hipEvent_t a = nullptr, b = nullptr;
    explicit CallTimer(bool on) {
        if (!on) return;
        HIP_CHECK(hipEventCreate(&a));
        HIP_CHECK(hipEventCreate(&b));
        HIP_CHECK(hipEventRecord(a, current_stream()));
    }
    ~CallTimer() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
    double stop() {
        if (!a) return 0.0;
        HIP_CHECK(hipEventRecord(b, current_stream()));
        HIP_CHECK(hipEventSynchronize(b));
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, a, b));
        return ms;
    }
};

}  // namespace

void run_with_mapping_best_path(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mp, double *out_logp,
                                uint32_t *out_path, uint32_t *out_counts, RowSink *sink) {
    hipStream_t s = current_stream();
    CallStats &st = stats();
    st = CallStats();
    const uint64_t R = reads->R, n_pos = reads->total;
    const uint32_t N = m->N, E = m->E;
    if (m->dev.max_degree > 8)
        PHMM_THROW(PHMM_EINVAL, "sparse path supports node degree <= 8 (MultiDbg MAX_DEGREE is 5)");
    for (uint64_t r = 0; r < R; r++)
        if (mp->read_max_list[r] > (uint32_t)PHMM_MAX_ACTIVE_NODES)
            PHMM_THROW(PHMM_ECAPACITY, "a mapping position lists more than 400 nodes");
    const uint32_t stride = (uint32_t)m->params.n_max_gaps + 2;
    upload_reads(reads);
    upload_mappings(mp);
    CallTimer tm(timing_enabled());

    // the model's init and trans as it was given them (natural logs), and the control arrays of the call
    WorkSet &ws = m->wset();
    DevBuf &d_init = ws.aux[7], &d_trans = ws.aux[8], &ctl = ws.aux[3], &recs = ws.aux[1], &rows = ws.aux[5];
    d_init.upload(m->init_logp.data(), sizeof(double) * N);
    d_trans.upload(m->trans_logp.data(), sizeof(double) * E);
    size_t cb = 0;
    auto carve = [&](size_t bytes) {
        cb = (cb + 255) / 256 * 256;
        const size_t o = cb;
        cb += bytes;
        return o;
    };
    const size_t o_logp = carve(sizeof(double) * R), o_ent = carve(sizeof(uint64_t) * (R + 1)),
                 o_end = carve(sizeof(uint32_t) * R), o_err = carve(sizeof(uint32_t) * R),
                 o_ids = carve(sizeof(uint32_t) * R), o_cnt = carve(sizeof(uint32_t) * 4 * R);
    ctl.reserve(cb);
    char *cp = ctl.as<char>();

    BestPathArgs a{};
    a.emis = m->dev.emis.as<uint8_t>();
    a.par_off = m->dev.par_off.as<uint32_t>();
    a.par_node = m->dev.par_node.as<uint32_t>();
    a.par_edge = m->dev.par_edge.as<uint32_t>();
    a.init_log = d_init.as<double>();
    a.trans_log = d_trans.as<double>();
    const phmm_params &pp = m->params;
    a.lp = BpParams{pp.p_mismatch, pp.p_match, pp.p_random, pp.p_end, pp.p_MM, pp.p_IM, pp.p_DM, pp.p_MI,
                    pp.p_II,       pp.p_DI,    pp.p_MD,     pp.p_ID,  pp.p_DD, (int)pp.n_max_gaps};
    a.bases = reads->d_bases.as<uint8_t>();
    a.read_off = reads->d_off.as<uint64_t>();
    a.map_pos_off = mp->d_pos_off.as<uint64_t>();
    a.map_nodes = mp->d_nodes.as<uint32_t>();
    a.read_ids = (const uint32_t *)(cp + o_ids);
    a.logp = (double *)(cp + o_logp);
    a.end_state = (uint32_t *)(cp + o_end);
    a.err = (uint32_t *)(cp + o_err);
    a.counts = (uint32_t *)(cp + o_cnt);
    a.stride = stride;

    // first entry of every read: the lists may live on the device only
    std::vector<uint64_t> ent(R + 1);
    hipLaunchKernelGGL(best_path_entry_offsets, dim3((unsigned)((R + 256) / 256)), dim3(256), 0, s, a.read_off,
                       a.map_pos_off, R, (uint64_t *)(cp + o_ent));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(ent.data(), cp + o_ent, sizeof(uint64_t) * (R + 1), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));

    const bool stage_rows = sink ? n_pos != 0 : out_path && n_pos && !is_device_pointer(out_path);
    const uint64_t fixed = cb + sizeof(double) * ((uint64_t)N + E), limit = table_budget(*m->pool);
    const uint64_t budget = limit > fixed ? limit - fixed : 0;
    auto read_bytes = [&](uint64_t r) {
        return sizeof(uint4) * (ent[r + 1] - ent[r]) +
               (stage_rows ? sizeof(uint32_t) * stride * (reads->off[r + 1] - reads->off[r]) : 0);
    };
    std::vector<uint32_t> ids;
    trace("best path setup");
    for (uint64_t r0 = 0; r0 < R;) {
        uint64_t r1 = r0, bytes = 0;
        while (r1 < R && (r1 == r0 || bytes + read_bytes(r1) <= budget)) bytes += read_bytes(r1++);
        const uint64_t n_ent = ent[r1] - ent[r0], n_rows = reads->off[r1] - reads->off[r0];
        recs.reserve(sizeof(uint4) * std::max<uint64_t>(n_ent, 1));
        if (stage_rows) rows.reserve(sizeof(uint32_t) * stride * std::max<uint64_t>(n_rows, 1));
        a.ent0 = ent[r0];
        a.rec = recs.as<uint4>();
        a.r0 = (uint32_t)r0;
        a.r1 = (uint32_t)r1;
        a.row0 = stage_rows ? reads->off[r0] : 0;
        a.path = stage_rows ? rows.as<uint32_t>() : out_path;
        for (int c = 0; c < 2; c++) {
            ids.clear();
            for (uint64_t r = r0; r < r1; r++)
                if ((mp->read_max_list[r] <= 64) == (c == 0)) ids.push_back((uint32_t)r);
            if (ids.empty()) continue;
            HIP_CHECK(hipMemcpyAsync(cp + o_ids, ids.data(), sizeof(uint32_t) * ids.size(), hipMemcpyHostToDevice, s));
            if (c == 0) hipLaunchKernelGGL((best_path_forward_kernel<64, 128>), dim3((unsigned)ids.size()), dim3(64), 0, s, a);
            else hipLaunchKernelGGL((best_path_forward_kernel<PHMM_MAX_ACTIVE_NODES, 1024>), dim3((unsigned)ids.size()), dim3(64), 0, s, a);
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipStreamSynchronize(s));  // the id list is reused by the next class
            st.launches[2]++;
        }
        trace("best path forward");
        hipLaunchKernelGGL(best_path_traceback_kernel, dim3((unsigned)((r1 - r0 + 63) / 64)), dim3(64), 0, s, a);
        HIP_CHECK(hipGetLastError());
        st.launches[2]++;
        if (sink) sink->chunk(r0, r1, stage_rows ? rows.as<uint32_t>() : nullptr, n_rows, stride);
        else if (stage_rows && n_rows)
            HIP_CHECK(hipMemcpyAsync(out_path + reads->off[r0] * stride, rows.p, sizeof(uint32_t) * stride * n_rows,
                                     hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        trace("best path traceback");
        r0 = r1;
    }
    st.ms[2] += tm.stop();
    st.cells[2] = mp->total_entries;
    {
        std::vector<uint32_t> herr(R);
        HIP_CHECK(hipMemcpy(herr.data(), a.err, sizeof(uint32_t) * R, hipMemcpyDeviceToHost));
        for (uint64_t r = 0; r < R; r++)
            if (herr[r]) PHMM_THROW(PHMM_EINTERNAL, "best path pass error " + std::to_string(herr[r]) + " (read " +
                                                        std::to_string(r) + ")");
    }
    copy_out(out_logp, a.logp, sizeof(double) * R);
    copy_out(out_counts, a.counts, sizeof(uint32_t) * 4 * R);
    trace("best path outputs");
}

}  // namespace phmm
