// phmm_run_with_mapping_tables: the forward and the backward table of every read over its mapping lists, written out per
// list entry and per base (list_tables_kernel.h).
//
// Host flow, as best_path.hip.  The reads are cut into chunks of consecutive reads whose staged outputs fit the workspace
// budget (phmm_set_workspace_limit; table_budget otherwise): an output the caller holds on the device is written in
// place, a host output goes through a staging buffer of the workspace (24 bytes per list entry and table, 16 per base and
// table) and is copied out chunk by chunk.  Per chunk: the forward kernel of the <= 64 class, the backward kernels of both
// classes, then -- once the forward's error words are back -- the forward kernel of the 400 class over its own reads and
// those of the small class that had more in-list parents than its link slots hold (SP_ERR_LINKS), then the wide-range
// forward kernel over the reads on which the scaled one lost range (LT_ERR_RANGE: a read cut by a k-mer of copy number 0;
// none on ordinary reads, and then nothing is launched).  A half none of whose outputs is asked for is not launched.  A read's values depend on the read and its lists alone, so the chunking shows
// nowhere.  The staging buffers are given back when the call ends.
#include <algorithm>
#include <cstring>

#include "list_tables_kernel.h"

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

struct StagingLease {  // the staging buffers go back to the device when the call ends, however it ends
    DevBuf &ent, &scal;
    ~StagingLease() {
        (void)hipStreamSynchronize(current_stream());
        ent.release();
        scal.release();
    }
};

// one output plane: where the kernels write it and, if that is a staging buffer, where it goes from there
struct Plane {
    double *user = nullptr;
    bool staged = false;
};

}  // namespace

void run_with_mapping_tables(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mp, double *out_lf, double *out_lb,
                             double *out_f, double *out_fs, double *out_b, double *out_bs) {
    hipStream_t s = current_stream();
    CallStats &st = stats();
    st = CallStats();
    const uint64_t R = reads->R;
    if (m->dev.max_degree > 8)
        PHMM_THROW(PHMM_EINVAL, "sparse path supports node degree <= 8 (MultiDbg MAX_DEGREE is 5)");
    for (uint64_t r = 0; r < R; r++)
        if (mp->read_max_list[r] > (uint32_t)PHMM_MAX_ACTIVE_NODES)
            PHMM_THROW(PHMM_ECAPACITY, "a mapping position lists more than 400 nodes");
    const bool want_f = out_lf || out_f || out_fs, want_b = out_lb || out_b || out_bs;
    if (!want_f && !want_b) return;
    upload_reads(reads);
    upload_mappings(mp);
    ensure_logib(m, reads->max_len + 1);
    CallTimer tm(timing_enabled());

    WorkSet &ws = m->wset();
    DevBuf &ctl = ws.aux[3], &st_ent = ws.aux[1], &st_scal = ws.aux[5];
    StagingLease lease{st_ent, st_scal};
    size_t cb = 0;
    auto carve = [&](size_t bytes) {
        cb = (cb + 255) / 256 * 256;
        const size_t o = cb;
        cb += bytes;
        return o;
    };
    const size_t o_lf = carve(sizeof(double) * R), o_lb = carve(sizeof(double) * R), o_ent = carve(sizeof(uint64_t) * (R + 1)),
                 o_ef = carve(sizeof(uint32_t) * R), o_eb = carve(sizeof(uint32_t) * R);
    size_t o_ids[3];  // reads of the small class, of the 400 class, and the 400 class plus the forward's promoted reads
    for (size_t &o : o_ids) o = carve(sizeof(uint32_t) * R);
    ctl.reserve(cb);
    char *cp = ctl.as<char>();

    ListTablesArgs base{};
    base.M = sparse_model_of(m);
    base.bases = reads->d_bases.as<uint8_t>();
    base.read_off = reads->d_off.as<uint64_t>();
    base.map_pos_off = mp->d_pos_off.as<uint64_t>();
    base.map_nodes = mp->d_nodes.as<uint32_t>();

    // first entry of every read: the lists may live on the device only
    std::vector<uint64_t> ent(R + 1);
    hipLaunchKernelGGL(list_tables_entry_offsets, dim3((unsigned)((R + 256) / 256)), dim3(256), 0, s, base.read_off,
                       base.map_pos_off, R, (uint64_t *)(cp + o_ent));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(ent.data(), cp + o_ent, sizeof(uint64_t) * (R + 1), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));

    // planes 0, 1: entries of the forward, the backward table; 2, 3: their scalars
    Plane pl[4];
    double *const users[4] = {out_f, out_b, out_fs, out_bs};
    uint64_t per_entry = 0, per_base = 0;
    for (int k = 0; k < 4; k++) {
        pl[k].user = users[k];
        pl[k].staged = users[k] && !is_device_pointer(users[k]);
        if (pl[k].staged) (k < 2 ? per_entry : per_base) += sizeof(double) * (k < 2 ? 3 : 2);
    }
    const uint64_t limit = table_budget(*m->pool);
    const uint64_t budget = limit > cb ? limit - cb : 0;
    auto read_bytes = [&](uint64_t r) {
        return per_entry * (ent[r + 1] - ent[r]) + per_base * (reads->off[r + 1] - reads->off[r]);
    };
    std::vector<uint32_t> ids[3], herr;
    trace("list tables setup");
    for (uint64_t r0 = 0; r0 < R;) {
        uint64_t r1 = r0, bytes = 0;
        while (r1 < R && (r1 == r0 || bytes + read_bytes(r1) <= budget)) bytes += read_bytes(r1++);
        const uint64_t n_ent = ent[r1] - ent[r0], n_rows = reads->off[r1] - reads->off[r0];
        if (per_entry) st_ent.reserve(std::max<uint64_t>(per_entry * n_ent, 1));
        if (per_base) st_scal.reserve(std::max<uint64_t>(per_base * n_rows, 1));
        // the kernels' view of plane k in this chunk
        double *dst[4];
        {
            double *pe = st_ent.as<double>(), *pb = st_scal.as<double>();
            for (int k = 0; k < 4; k++) {
                dst[k] = pl[k].user;
                if (!pl[k].staged) continue;
                if (k < 2) {
                    dst[k] = pe;
                    pe += 3 * n_ent;
                } else {
                    dst[k] = pb;
                    pb += 2 * n_rows;
                }
            }
        }
        auto args_of = [&](bool fwd, int id_slot) {
            ListTablesArgs a = base;
            const int ke = fwd ? 0 : 1, ks = fwd ? 2 : 3;
            a.ent = dst[ke];
            a.scal = dst[ks];
            a.ent0 = pl[ke].staged ? ent[r0] : 0;
            a.row0 = pl[ks].staged ? reads->off[r0] : 0;
            a.logp = (double *)(cp + (fwd ? o_lf : o_lb));
            a.err = (uint32_t *)(cp + (fwd ? o_ef : o_eb));
            a.read_ids = (const uint32_t *)(cp + o_ids[id_slot]);
            return a;
        };
        auto put_ids = [&](int slot) {
            if (!ids[slot].empty())
                HIP_CHECK(hipMemcpyAsync(cp + o_ids[slot], ids[slot].data(), sizeof(uint32_t) * ids[slot].size(),
                                         hipMemcpyHostToDevice, s));
        };
        auto launch = [&](bool fwd, bool big, int id_slot, bool wide_range = false) {
            const unsigned nb = (unsigned)ids[id_slot].size();
            if (!nb) return;
            const ListTablesArgs a = args_of(fwd, id_slot);
            if (wide_range && !big) hipLaunchKernelGGL((list_tables_forward_wide_kernel<64, 256>), dim3(nb), dim3(64), 0, s, a);
            else if (wide_range)
                hipLaunchKernelGGL((list_tables_forward_wide_kernel<PHMM_MAX_ACTIVE_NODES, 1024>), dim3(nb), dim3(64), 0, s, a);
            else if (fwd && !big) hipLaunchKernelGGL((list_tables_forward_kernel<64, 2>), dim3(nb), dim3(64), 0, s, a);
            else if (fwd) hipLaunchKernelGGL((list_tables_forward_kernel<PHMM_MAX_ACTIVE_NODES, 8>), dim3(nb), dim3(64), 0, s, a);
            else if (!big) hipLaunchKernelGGL((list_tables_backward_kernel<64>), dim3(nb), dim3(64), 0, s, a);
            else hipLaunchKernelGGL((list_tables_backward_kernel<PHMM_MAX_ACTIVE_NODES>), dim3(nb), dim3(64), 0, s, a);
            HIP_CHECK(hipGetLastError());
            st.launches[2]++;
        };
        auto forward_errors = [&] {  // the forward's error words of the chunk's reads, behind everything launched so far
            herr.resize(r1 - r0);
            HIP_CHECK(hipMemcpyAsync(herr.data(), cp + o_ef + sizeof(uint32_t) * r0, sizeof(uint32_t) * (r1 - r0),
                                     hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipStreamSynchronize(s));
        };
        for (auto &v : ids) v.clear();
        for (uint64_t r = r0; r < r1; r++) ids[mp->read_max_list[r] <= 64 ? 0 : 1].push_back((uint32_t)r);
        put_ids(0);
        put_ids(1);
        if (want_f) launch(true, false, 0);
        if (want_b) {
            launch(false, false, 0);
            launch(false, true, 1);
        }
        if (want_f) {
            ids[2] = ids[1];
            if (!ids[0].empty()) {
                // the small class's reads that need more link slots run again in the 400 class, which has 8 per node
                forward_errors();
                for (uint32_t r : ids[0])
                    if (herr[r - r0] == SP_ERR_LINKS) ids[2].push_back(r);
            }
            put_ids(2);
            launch(true, true, 2);
            // the reads on which the scaled forward lost range (LT_ERR_RANGE): again with an exponent per value.  The id
            // lists of the two classes are free by now: every kernel that read them has ended.
            forward_errors();
            ids[0].clear();
            ids[1].clear();
            for (uint64_t r = r0; r < r1; r++)
                if (herr[r - r0] == LT_ERR_RANGE) ids[mp->read_max_list[r] <= 64 ? 0 : 1].push_back((uint32_t)r);
            put_ids(0);
            put_ids(1);
            launch(true, false, 0, true);
            launch(true, true, 1, true);
        }
        trace("list tables kernels");
        for (int k = 0; k < 4; k++) {
            if (!pl[k].staged) continue;
            const uint64_t n = k < 2 ? 3 * n_ent : 2 * n_rows, at = k < 2 ? 3 * ent[r0] : 2 * reads->off[r0];
            if (n) HIP_CHECK(hipMemcpyAsync(pl[k].user + at, dst[k], sizeof(double) * n, hipMemcpyDeviceToHost, s));
        }
        HIP_CHECK(hipStreamSynchronize(s));  // (the id lists and the staging buffers are reused by the next chunk)
        trace("list tables outputs");
        r0 = r1;
    }
    st.ms[2] += tm.stop();
    st.cells[2] = mp->total_entries;
    {
        std::vector<uint32_t> ef(R, 0), eb(R, 0);
        if (want_f) HIP_CHECK(hipMemcpy(ef.data(), cp + o_ef, sizeof(uint32_t) * R, hipMemcpyDeviceToHost));
        if (want_b) HIP_CHECK(hipMemcpy(eb.data(), cp + o_eb, sizeof(uint32_t) * R, hipMemcpyDeviceToHost));
        for (uint64_t r = 0; r < R; r++)
            if ((ef[r] | eb[r]) & SP_ERR_DUPLICATE)
                PHMM_THROW(PHMM_EINVAL, "duplicate node in a mapping list (read " + std::to_string(r) + ")");
        for (uint64_t r = 0; r < R; r++)
            if (ef[r] | eb[r])
                PHMM_THROW(PHMM_EINTERNAL, "list tables pass error " + std::to_string(ef[r] | eb[r]) + " (read " +
                                               std::to_string(r) + ")");
    }
    if (want_f) copy_out(out_lf, cp + o_lf, sizeof(double) * R);
    if (want_b) copy_out(out_lb, cp + o_lb, sizeof(double) * R);
    trace("list tables totals");
}

}  // namespace phmm
