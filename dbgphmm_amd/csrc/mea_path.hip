// phmm_run_with_mapping_weighted_path and phmm_run_with_mapping_mea_path (include/phmm_amd_mea.h): the max-sum pass
// over mapping lists with per-entry weights and its traceback (mea_path_kernel.h, best_path_kernel.h).
//
// Host flow of the weighted walk: that of best_path.hip.  The weights (24 bytes per entry) and the InsBegin weights
// (8 bytes per base) of a host caller are uploaded once, into workspace buffers the states pass does not use; a device
// check pass refuses a NaN or an infinity before the first forward launch.  The reads are then cut into chunks of
// consecutive reads whose back-pointer records (16 bytes per list entry) and, for a host out_path, staged rows fit the
// workspace budget (phmm_set_workspace_limit; table_budget otherwise).  Per chunk: the forward kernel of the <= 64
// class and of the 400 class, the traceback of the best path over all of the chunk's reads, then the rows go out -- or,
// with a RowSink, are handed over on the device.  Score and counts of all reads stay in the workspace until the last
// chunk is done.
//
// The MEA call runs run_with_mapping_states with the weights plane as its device output, turns the plane into weights
// in place with one kernel and walks it as above: no posterior leaves the device unless out_weights asks for it.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "mea_path_kernel.h"

namespace phmm {

namespace {

bool mea_is_device_pointer(const void *p) {
    hipPointerAttribute_t at;
    const bool dev = hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeDevice;
    if (!dev) (void)hipGetLastError();
    return dev;
}

struct MeaTimer {  // device time of the walk on its stream (index 2 of phmm_last_call_stats)
    hipEvent_t a = nullptr, b = nullptr;
    explicit MeaTimer(bool on) {
        if (!on) return;
        HIP_CHECK(hipEventCreate(&a));
        HIP_CHECK(hipEventCreate(&b));
        HIP_CHECK(hipEventRecord(a, current_stream()));
    }
    ~MeaTimer() {
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

void check_lists(const phmm_model *m, const phmm_reads *reads, const phmm_mappings *mp) {
    if (m->dev.max_degree > 8)
        PHMM_THROW(PHMM_EINVAL, "sparse path supports node degree <= 8 (MultiDbg MAX_DEGREE is 5)");
    for (uint64_t r = 0; r < reads->R; r++)
        if (mp->read_max_list[r] > (uint32_t)PHMM_MAX_ACTIVE_NODES)
            PHMM_THROW(PHMM_ECAPACITY, "a mapping position lists more than 400 nodes");
}

// d_w: the weights on the device (checked here), d_ib: the InsBegin weights on the device or null
void weighted_walk(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mp, const double *d_w, const double *d_ib,
                   uint64_t plane_bytes, double *out_score, uint32_t *out_path, uint32_t *out_counts, RowSink *sink) {
    hipStream_t s = current_stream();
    CallStats &st = stats();
    const uint64_t R = reads->R, n_pos = reads->total, n_ent = mp->total_entries;
    const uint32_t N = m->N, E = m->E;
    const uint32_t stride = (uint32_t)m->params.n_max_gaps + 2;
    MeaTimer tm(timing_enabled());

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
                 o_ids = carve(sizeof(uint32_t) * R), o_cnt = carve(sizeof(uint32_t) * 4 * R),
                 o_flag = carve(sizeof(uint32_t));
    ctl.reserve(cb);
    char *cp = ctl.as<char>();

    // no NaN, no infinity: before the first forward launch
    {
        uint32_t *flag = (uint32_t *)(cp + o_flag), h = 0;
        HIP_CHECK(hipMemsetAsync(flag, 0, sizeof(uint32_t), s));
        auto blocks = [](uint64_t n) { return dim3((unsigned)std::min<uint64_t>((n + 255) / 256, 4096)); };
        if (n_ent) hipLaunchKernelGGL(mea_check_weights, blocks(3 * n_ent), dim3(256), 0, s, d_w, 3 * n_ent, flag);
        if (d_ib && n_pos) hipLaunchKernelGGL(mea_check_weights, blocks(n_pos), dim3(256), 0, s, d_ib, n_pos, flag);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(&h, flag, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (h) PHMM_THROW(PHMM_EINVAL, "a weight is NaN or infinite");
    }

    MeaArgs ma{};
    BestPathArgs &a = ma.b;
    ma.weights = d_w;
    ma.ib_weight = d_ib;
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

    const bool stage_rows = sink ? n_pos != 0 : out_path && n_pos && !mea_is_device_pointer(out_path);
    const uint64_t fixed = cb + sizeof(double) * ((uint64_t)N + E) + plane_bytes, limit = table_budget(*m->pool);
    const uint64_t budget = limit > fixed ? limit - fixed : 0;
    auto read_bytes = [&](uint64_t r) {
        return sizeof(uint4) * (ent[r + 1] - ent[r]) +
               (stage_rows ? sizeof(uint32_t) * stride * (reads->off[r + 1] - reads->off[r]) : 0);
    };
    std::vector<uint32_t> ids;
    trace("weighted path setup");
    for (uint64_t r0 = 0; r0 < R;) {
        uint64_t r1 = r0, bytes = 0;
        while (r1 < R && (r1 == r0 || bytes + read_bytes(r1) <= budget)) bytes += read_bytes(r1++);
        const uint64_t c_ent = ent[r1] - ent[r0], n_rows = reads->off[r1] - reads->off[r0];
        recs.reserve(sizeof(uint4) * std::max<uint64_t>(c_ent, 1));
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
            if (c == 0) hipLaunchKernelGGL((mea_forward_kernel<64, 128>), dim3((unsigned)ids.size()), dim3(64), 0, s, ma);
            else hipLaunchKernelGGL((mea_forward_kernel<PHMM_MAX_ACTIVE_NODES, 1024>), dim3((unsigned)ids.size()), dim3(64), 0, s, ma);
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipStreamSynchronize(s));  // the id list is reused by the next class
            st.launches[2]++;
        }
        trace("weighted path forward");
        hipLaunchKernelGGL(best_path_traceback_kernel, dim3((unsigned)((r1 - r0 + 63) / 64)), dim3(64), 0, s, a);
        HIP_CHECK(hipGetLastError());
        st.launches[2]++;
        if (sink) sink->chunk(r0, r1, stage_rows ? rows.as<uint32_t>() : nullptr, n_rows, stride);
        else if (stage_rows && n_rows)
            HIP_CHECK(hipMemcpyAsync(out_path + reads->off[r0] * stride, rows.p, sizeof(uint32_t) * stride * n_rows,
                                     hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        trace("weighted path traceback");
        r0 = r1;
    }
    st.ms[2] += tm.stop();
    st.cells[2] = n_ent;
    {
        std::vector<uint32_t> herr(R);
        HIP_CHECK(hipMemcpy(herr.data(), a.err, sizeof(uint32_t) * R, hipMemcpyDeviceToHost));
        for (uint64_t r = 0; r < R; r++)
            if (herr[r]) PHMM_THROW(PHMM_EINTERNAL, "weighted path pass error " + std::to_string(herr[r]) + " (read " +
                                                        std::to_string(r) + ")");
    }
    copy_out(out_score, a.logp, sizeof(double) * R);
    copy_out(out_counts, a.counts, sizeof(uint32_t) * 4 * R);
    trace("weighted path outputs");
}

}  // namespace

void run_with_mapping_weighted_path(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mp, const double *weights,
                                    const double *ib_weight, double *out_score, uint32_t *out_path, uint32_t *out_counts,
                                    RowSink *sink) {
    hipStream_t s = current_stream();
    stats() = CallStats();
    check_lists(m, reads, mp);
    if (!weights) PHMM_THROW(PHMM_EINVAL, "weights is NULL");
    const uint64_t n_ent = mp->total_entries, n_pos = reads->total;
    upload_reads(reads);
    upload_mappings(mp);
    // host weights go up once; device weights are read where they are
    WorkSet &ws = m->wset();
    DevBuf &d_w = ws.aux[0], &d_ib = ws.aux[22];
    uint64_t plane = 0;
    const double *w = weights, *ib = ib_weight;
    if (n_ent && !mea_is_device_pointer(weights)) {
        plane += sizeof(double) * 3 * n_ent;
        d_w.reserve(sizeof(double) * 3 * n_ent);
        HIP_CHECK(hipMemcpyAsync(d_w.p, weights, sizeof(double) * 3 * n_ent, hipMemcpyHostToDevice, s));
        w = d_w.as<double>();
    }
    if (ib_weight && n_pos && !mea_is_device_pointer(ib_weight)) {
        plane += sizeof(double) * n_pos;
        d_ib.reserve(sizeof(double) * n_pos);
        HIP_CHECK(hipMemcpyAsync(d_ib.p, ib_weight, sizeof(double) * n_pos, hipMemcpyHostToDevice, s));
        ib = d_ib.as<double>();
    }
    HIP_CHECK(hipStreamSynchronize(s));  // (the caller's host arrays are free again)
    weighted_walk(m, reads, mp, w, ib, plane, out_score, out_path, out_counts, sink);
}

void run_with_mapping_mea_path(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mp, double del_weight,
                               double *out_lf, double *out_score, uint32_t *out_path, uint32_t *out_counts,
                               double *out_weights, RowSink *sink) {
    hipStream_t s = current_stream();
    if (!(del_weight >= 0.0) || std::isinf(del_weight)) PHMM_THROW(PHMM_EINVAL, "del_weight must be finite and >= 0");
    check_lists(m, reads, mp);
    const uint64_t R = reads->R, n_ent = mp->total_entries, plane = sizeof(double) * 3 * n_ent;
    if (plane > table_budget(*m->pool))
        PHMM_THROW(PHMM_ECAPACITY, "the weights plane (24 bytes per list entry) exceeds the workspace limit");
    DevBuf &d_w = m->wset().aux[0];
    d_w.reserve(std::max<uint64_t>(plane, 8));
    // the posteriors by state, written in place on the device (its refusals come before any of its writes)
    std::vector<double> lf(R);
    run_with_mapping_states(m, reads, mp, lf.data(), n_ent ? d_w.as<double>() : nullptr, nullptr);
    {  // index 2 counts the walk alone; the other indices stay those of the states pass
        CallStats &st = stats();
        st.ms[2] = 0.0;
        st.launches[2] = st.cells[2] = 0;
    }
    if (n_ent) {
        hipLaunchKernelGGL(mea_weights_from_states, dim3((unsigned)std::min<uint64_t>((3 * n_ent + 255) / 256, 4096)),
                           dim3(256), 0, s, d_w.as<double>(), 3 * n_ent, del_weight);
        HIP_CHECK(hipGetLastError());
    }
    weighted_walk(m, reads, mp, d_w.as<double>(), nullptr, plane, out_score, out_path, out_counts, sink);
    if (out_weights && n_ent) copy_out(out_weights, d_w.p, plane);
    put_doubles(out_lf, lf.data(), R);
    trace("mea path outputs");
}

}  // namespace phmm
