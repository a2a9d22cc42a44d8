// phmm_run_with_mapping_alignments: the best path or the sampled paths of every read as alignment records
// (include/phmm_amd_align.h; kernels in alignments_kernel.h).
//
// Host flow.  The call is run_with_mapping_best_path (n_samples == 0) or run_with_mapping_sample_paths with a RowSink:
// the parent cuts the reads into chunks, runs its forward and walk kernels and leaves the chunk's rows in the workspace
// (aux[5]); the sink compacts them before the next chunk overwrites them.  Per chunk:
//   1. the count kernel: the CIGAR words and the walk runs of every alignment of the chunk;
//   2. an exclusive scan of each (hipcub), started at the totals of the chunks before, straight into the handle's
//      offset arrays -- chunks hold whole reads and alignments are read-major, so a chunk's alignments are contiguous;
//   3. the two totals come back to the host and the handle's three word arrays grow to them (a device copy keeps what
//      the earlier chunks wrote; a call of one chunk allocates each array once, at its final size);
//   4. the write kernel stores the words.
// The counts and the scan's scratch are workspace buffers (aux[9], aux[10]); what the handle owns is its own.
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "alignments_kernel.h"

namespace phmm {

namespace {

struct AlignSink final : RowSink {
    phmm_model *m;
    const phmm_reads *reads;
    const phmm_mappings *mp;
    uint32_t planes;
    phmm_alignments *h;
    uint64_t ops_done = 0, runs_done = 0;

    void chunk(uint64_t r0, uint64_t r1, const uint32_t *rows, uint64_t plane_rows, uint32_t stride) override {
        hipStream_t s = current_stream();
        CallStats &st = stats();
        trace("alignments rows");  // (the parent's walk: its own mark comes behind the sink)
        const uint64_t n_aln = (r1 - r0) * planes, a0 = r0 * planes;
        if (n_aln + 1 > (uint64_t)INT32_MAX) PHMM_THROW(PHMM_ECAPACITY, "more than 2^31 - 2 alignments in one chunk");
        WorkSet &ws = m->wset();
        DevBuf &cnt = ws.aux[9], &tmp = ws.aux[10];
        cnt.reserve(sizeof(uint64_t) * 2 * (n_aln + 1));
        uint64_t *c_ops = cnt.as<uint64_t>(), *c_runs = c_ops + n_aln + 1;
        HIP_CHECK(hipMemsetAsync(c_ops + n_aln, 0, sizeof(uint64_t), s));
        HIP_CHECK(hipMemsetAsync(c_runs + n_aln, 0, sizeof(uint64_t), s));

        AlignArgs a{};
        a.emis = m->dev.emis.as<uint8_t>();
        a.n_nodes = m->N;
        a.bases = reads->d_bases.as<uint8_t>();
        a.read_off = reads->d_off.as<uint64_t>();
        a.map_pos_off = mp->d_pos_off.as<uint64_t>();
        a.map_nodes = mp->d_nodes.as<uint32_t>();
        a.rows = rows;
        a.row0 = reads->off[r0];
        a.plane_rows = plane_rows;
        a.stride = stride;
        a.r0 = (uint32_t)r0;
        a.planes = planes;
        a.n_aln = n_aln;
        a.cnt_ops = c_ops;
        a.cnt_runs = c_runs;
        const dim3 grid((unsigned)((n_aln + AL_WAVES - 1) / AL_WAVES)), block(64 * AL_WAVES);
        hipLaunchKernelGGL(alignments_kernel<false>, grid, block, 0, s, a);
        HIP_CHECK(hipGetLastError());
        st.launches[2]++;
        trace("alignments count");

        uint64_t *op_off = h->d_op_off.as<uint64_t>() + a0, *run_off = h->d_run_off.as<uint64_t>() + a0;
        size_t tb = 0;
        HIP_CHECK(hipcub::DeviceScan::ExclusiveScan(nullptr, tb, c_ops, op_off, hipcub::Sum(), ops_done, (int)(n_aln + 1), s));
        tmp.reserve(tb);
        HIP_CHECK(hipcub::DeviceScan::ExclusiveScan(tmp.p, tb, c_ops, op_off, hipcub::Sum(), ops_done, (int)(n_aln + 1), s));
        HIP_CHECK(hipcub::DeviceScan::ExclusiveScan(tmp.p, tb, c_runs, run_off, hipcub::Sum(), runs_done, (int)(n_aln + 1), s));
        uint64_t tot[2];
        HIP_CHECK(hipMemcpyAsync(&tot[0], op_off + n_aln, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(&tot[1], run_off + n_aln, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        trace("alignments scan");

        grow_keep(h->d_ops, sizeof(uint32_t) * ops_done, sizeof(uint32_t) * tot[0], s);
        grow_keep(h->d_run_node, sizeof(uint32_t) * runs_done, sizeof(uint32_t) * tot[1], s);
        grow_keep(h->d_run_len, sizeof(uint32_t) * runs_done, sizeof(uint32_t) * tot[1], s);
        a.op_off = op_off;
        a.run_off = run_off;
        a.ops = h->d_ops.as<uint32_t>();
        a.run_node = h->d_run_node.as<uint32_t>();
        a.run_len = h->d_run_len.as<uint32_t>();
        hipLaunchKernelGGL(alignments_kernel<true>, grid, block, 0, s, a);
        HIP_CHECK(hipGetLastError());
        st.launches[2]++;
        ops_done = tot[0];
        runs_done = tot[1];
        trace("alignments write");
    }
};

}  // namespace

void run_with_mapping_alignments(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mp, uint32_t n_samples,
                                 uint64_t seed, double *out_logp, double *out_path_logp, uint32_t *out_counts,
                                 phmm_alignments *h) {
    AlignSink sink;
    sink.m = m;
    sink.reads = reads;
    sink.mp = mp;
    sink.planes = std::max<uint32_t>(n_samples, 1);
    sink.h = h;
    if (h) {
        h->A = reads->R * sink.planes;
        h->device = m->pool->device;
        h->d_op_off.reserve(sizeof(uint64_t) * (h->A + 1));
        h->d_run_off.reserve(sizeof(uint64_t) * (h->A + 1));
    }
    RowSink *rs = h ? &sink : nullptr;
    if (n_samples == 0) run_with_mapping_best_path(m, reads, mp, out_logp, nullptr, out_counts, rs);
    else run_with_mapping_sample_paths(m, reads, mp, n_samples, seed, out_logp, out_path_logp, nullptr, out_counts, nullptr, rs);
    if (h) {
        h->total_ops = sink.ops_done;
        h->total_runs = sink.runs_done;
    }
}

void alignments_export(const phmm_alignments *h, uint64_t *op_off, uint32_t *ops, uint64_t *run_off, uint32_t *run_node,
                       uint32_t *run_len) {
    if (h->A == 0) {  // (a call without reads: nothing on the device)
        const uint64_t zero = 0;
        put_bytes(op_off, &zero, sizeof zero);
        put_bytes(run_off, &zero, sizeof zero);
        return;
    }
    copy_out(op_off, h->d_op_off.p, sizeof(uint64_t) * (h->A + 1));
    copy_out(run_off, h->d_run_off.p, sizeof(uint64_t) * (h->A + 1));
    copy_out(ops, h->d_ops.p, sizeof(uint32_t) * h->total_ops);
    copy_out(run_node, h->d_run_node.p, sizeof(uint32_t) * h->total_runs);
    copy_out(run_len, h->d_run_len.p, sizeof(uint32_t) * h->total_runs);
}

}  // namespace phmm
