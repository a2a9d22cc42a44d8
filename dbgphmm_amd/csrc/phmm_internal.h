// Internal declarations shared by the host side and the HIP kernels.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/phmm_amd.h"
#include "../../include/phmm_amd_states.h"
#include "../../include/phmm_amd_path.h"
#include "../../include/phmm_amd_share.h"
#include "../../include/phmm_amd_sample.h"
#include "../../include/phmm_amd_generate.h"
#include "../../include/phmm_amd_align.h"
#include "../../include/phmm_amd_mea.h"
#include "../../include/phmm_amd_tables.h"
#include "../../include/phmm_amd_usage.h"
#include "../../include/phmm_amd_edges.h"
#include "../../include/phmm_amd_pileup.h"

namespace phmm {

// ---------------------------------------------------------------- errors
void set_error(const std::string &msg);
int fail(int code, const std::string &msg);

struct Error {
    int code;
    std::string msg;
};
#define PHMM_THROW(code, msg) throw ::phmm::Error{(code), (msg)}
#define HIP_CHECK(expr)                                                                      \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess)                                                                \
            PHMM_THROW(_e == hipErrorOutOfMemory ? PHMM_ENOMEM : PHMM_ENODEVICE,             \
                       std::string(#expr) + ": " + hipGetErrorString(_e));                   \
    } while (0)

hipStream_t current_stream();
// workspace set of the calling thread (0 unless the thread is a pipeline worker)
int &workset_index();
// a pipeline worker adopts the API thread's per-call settings with its own stream and workspace set
struct ThreadContext {
    uint64_t ws_limit;
    bool timing;
    int device;
};
ThreadContext capture_thread_context();
void adopt_thread_context(const ThreadContext &c, hipStream_t stream, int workset);
uint64_t workspace_limit();
struct DevicePool;
// DP-table budget of a call: PHMM_MEM_FRACTION (0.9) of what is free plus the pool's own tables (they are
// re-allocated), less `reserve` bytes the call's other buffers still have to grow by
uint64_t table_budget(const DevicePool &pool, uint64_t reserve = 0);
// budget of a call that plans every buffer it uses (sparse_dyn.hip): a fraction of free + everything the pool holds
uint64_t planned_budget(const DevicePool &pool);

// ---------------------------------------------------------------- device buffers
void flush_spare_buffers();  // (api.cpp) frees the spare buffers of the current device's pool
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    // grow-only
    void reserve(size_t n) {
        if (n <= bytes) return;
        release();
        if (hipMalloc(&p, n ? n : 1) != hipSuccess) {
            // the spare result buffers (DevicePool::recycle) are the one thing this library holds that nobody needs
            (void)hipGetLastError();
            p = nullptr;
            flush_spare_buffers();
            HIP_CHECK(hipMalloc(&p, n ? n : 1));
        }
        bytes = n;
    }
    void adopt(void *q, size_t n) {
        release();
        p = q;
        bytes = n;
    }
    void *detach() {
        void *q = p;
        p = nullptr;
        bytes = 0;
        return q;
    }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
    void upload(const void *src, size_t n) {
        reserve(n);
        if (n) HIP_CHECK(hipMemcpyAsync(p, src, n, hipMemcpyHostToDevice, current_stream()));
    }
};
// copy device -> (host or device) destination
void copy_out(void *dst, const void *src_dev, size_t bytes);
// b holds at least `need` bytes and still its first `used` (the arrays a result handle grows chunk by chunk)
inline void grow_keep(DevBuf &b, size_t used, size_t need, hipStream_t s) {
    if (need <= b.bytes) return;
    DevBuf nb;
    nb.reserve(need > 2 * b.bytes ? need : 2 * b.bytes);
    if (used) HIP_CHECK(hipMemcpyAsync(nb.p, b.p, used, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));  // the old buffer is freed below
    const size_t n = nb.bytes;
    b.adopt(nb.detach(), n);
}

// ---------------------------------------------------------------- per-device workspace pool
// One set of grow-only buffers per pipeline worker (sparse_dyn.hip runs chunks of read groups concurrently on
// their own streams); the API thread and single-stream paths use set 0.  aux[] = per-call scratch kept across
// calls (no hipMalloc in the steady state).  phmm_release_workspace() gives everything back.
struct WorkSet {
    DevBuf tables, misc, aux[24];
    size_t bytes() const {
        size_t b = tables.bytes + misc.bytes;
        for (const auto &a : aux) b += a.bytes;
        return b;
    }
    void release() {
        tables.release();
        misc.release();
        for (auto &a : aux) a.release();
    }
};
static constexpr int MAX_WORKERS = 4;
struct DevicePool {
    int device = 0;
    std::recursive_mutex call_mu;  // compute calls on one device run one at a time (any handle, any thread)
    WorkSet wsets[MAX_WORKERS];
    hipStream_t wstream[MAX_WORKERS] = {};  // worker streams, created on first use
    hipStream_t cstream[MAX_WORKERS] = {};  // per worker: side stream of the mapping-list kernels (mapping_flow.hip)
    hipEvent_t cevent[MAX_WORKERS][4] = {};
    DevBuf ws_out;
    // The device buffers of destroyed phmm_mappings (their CSR: gigabytes on a tandem repeat), kept for the next
    // generate_mappings call: a hipFree + hipMalloc pair per buffer and call otherwise (0.1-2 s per call on `rep20`,
    // and it varies from box to box).  At most SPARE_MAX buffers / SPARE_BYTES; given back by release(), and by any
    // allocation that fails (DevBuf::reserve).
    static constexpr size_t SPARE_MAX = 6, SPARE_BYTES = (size_t)8 << 30;
    std::mutex spare_mu;
    std::vector<std::pair<void *, size_t>> spare;
    size_t spare_total = 0;
    void recycle(DevBuf &b);         // takes b's memory (frees it when the cache is full)
    void take(DevBuf &b, size_t n);  // b.reserve(n), out of the cache when a spare of n .. 2n bytes is there
    void flush_spares();
    size_t owned_table_bytes() const {
        size_t b = 0;
        for (const auto &w : wsets) b += w.tables.bytes;
        return b;
    }
    size_t owned_bytes() const {
        size_t b = ws_out.bytes + spare_total;
        for (const auto &w : wsets) b += w.bytes();
        return b;
    }
    void release();  // frees every buffer, stream and event (the device must be idle)
};
// the pool of the calling thread's current device (created on first use, never destroyed: HIP may be gone at exit)
DevicePool &device_pool();

// ---------------------------------------------------------------- linear-domain parameters
// The kernels run in the (scaled) linear probability domain; see DESIGN.md.
struct LinParams {
    double p_mismatch, p_match, p_random, p_end;
    double p_MM, p_IM, p_DM, p_MI, p_II, p_DI, p_MD, p_ID, p_DD;
    int n_max_gaps;
};

// ancestor closure entry (forward): node a reaches k in `hop` edges with path weight w.
//   w1 = w if hop==1 (direct parent: p_MM/p_IM terms)
//   wD = pDD^(hop-1) w  for hop <= G+1   -> d[k]      = sum wD * g[a] + c*dinit[k]
//   wT = pDD^(hop-2) w  for 2<=hop<=G+2  -> (T d)[k]  = sum wT * g[a] + c*tdinit[k]
// with g[a] = p_MD m[a] + p_ID i[a]   (forward.rs:423-524 unrolled; DESIGN.md "Del closure")
struct FwdEntry {
    uint32_t node;
    uint32_t pad;
    double w1, wD, wT;
};
// descendant closure entry (backward): v reaches u in `hop` edges with path weight w.
//   c1  = w if hop==1
//   cAd = pDD^(hop-1) w for hop <= G+1 ; cAt = pDD^(hop-2) w for 2<=hop<=G+2
//   cQd = pDD^hop w     for hop <= G      (cQt == cAd)
// (backward.rs:299-483 unrolled)
struct BwdEntry {
    uint32_t node;
    uint32_t emis;
    double c1, cAd, cAt, cQd;
};

// Closure entry by hop (n_max_gaps <= 4): node `node` reaches (is reached from) k in exactly `hop`
// edges with total path weight w.  The kernels keep, per thread, the per-hop sums
//   A[h] = sum over entries with hop h+1 of w * value(node)        h = 0 .. CHAIN_HOPS-1
// ("window") from which every Del-closure term follows with fixed coefficients (DenseArgs::cD ..).
struct HopEntry {
    uint32_t node;
    uint32_t hop_emis;  // hop | emission(node) << 8
    double w;
};

// Per-node record of the dense kernels (one 32-byte scalar load per node).
//   CHAIN_F: k's only parent is k-1 and that edge has weight 1 -> the window of k is the window of k-1
//            shifted by one hop with k-1's own values in front (no gather at all)
//   CHAIN_B: k's only child is k+1, weight 1 (the same for the descendant window)
// Node ids follow the k-mer order of the haplotypes, so this holds along unitigs AND behind a merge;
// the window is rebuilt from the hop entries at the first node of a thread's run, behind a branch and
// at a merge node only.  (n_max_gaps > 4: no flags, merged closure entries, no window.)
struct NodeRec {
    double init, dinit, tdinit;
    uint32_t emis;
    uint32_t flags;
};
static constexpr uint32_t CHAIN_F = 1u, CHAIN_B = 2u;
static constexpr int CHAIN_HOPS = 6;

// Everything the sparse (frontier) kernels need to know about one node, in ONE aligned record: a
// wave that meets a new node pays one memory round trip for it instead of the CSR's three dependent
// ones (offsets -> neighbour ids / weights -> their emissions).  Neighbours keep the CSR (petgraph)
// order.  MultiDbg bounds the degree by 5 (multi_dbg.rs:82); `over` marks nodes beyond that, which
// only the dense kernels support.
static constexpr int ADJ_DEG = 5;
struct alignas(16) FwdAdj {   // forward: expansion to children, sums over parents
    double par_w[ADJ_DEG];    // linear transition probability parent -> this node (the model's own)
    double init;
    uint32_t par[ADJ_DEG];
    uint32_t chi[ADJ_DEG];
    uint8_t emis, npar, nchi, over;
    uint32_t pad;
};
struct alignas(16) BwdAdj {   // backward: sums over children
    double chi_w[ADJ_DEG];
    uint32_t chi[ADJ_DEG];
    uint8_t chi_emis[ADJ_DEG];
    uint8_t emis, nchi, over;
    uint32_t par0;            // first parent (0xffffffff: none): the node a backward column takes in next on a unitig
    double init;              // Begin -> this node (the model's own): the Begin-state sums bmb / bib (backward.rs:499-555)
};
// Topology-only record of the hinted forward (candidate batches bring their own init / trans): parents with the
// ids of their edges, so that trans[candidate][edge] is one dependent load behind the record.
struct alignas(16) ParRec {
    uint32_t par[ADJ_DEG];
    uint32_t pedge[ADJ_DEG];
    uint8_t npar, emis, over, pad;
    uint32_t pad2;
};
static_assert(sizeof(FwdAdj) == 96 && sizeof(BwdAdj) == 80 && sizeof(ParRec) == 48, "adjacency record layout");

struct ModelDev {
    uint32_t N = 0, E = 0;
    DevBuf nodes;            // NodeRec[N]
    DevBuf emis;             // u8[N]
    DevBuf init;             // f64[N] linear
    DevBuf dinit, tdinit;    // f64[N]
    DevBuf fc_off, fc_ent;   // u32[N+1], FwdEntry[]
    DevBuf bc_off, bc_ent;   // u32[N+1], BwdEntry[]
    DevBuf fh_off, fh_ent;   // u32[N+1], HopEntry[]  (ancestors by hop)
    DevBuf bh_off, bh_ent;   // u32[N+1], HopEntry[]  (descendants by hop)
    // parent / child CSR in linear domain for the sparse kernels
    DevBuf par_off, par_node, par_w;  // u32[N+1], u32[E], f64[E]
    DevBuf chi_off, chi_node, chi_w;
    DevBuf par_edge, chi_edge;        // u32[E] edge ids (candidate batches index trans by edge)
    DevBuf trans_lin;                 // f64[E] by edge id
    DevBuf fadj, badj;                // FwdAdj[N], BwdAdj[N]
    DevBuf prec;                      // ParRec[N]
    DevBuf logib;                     // f64[logib_len] forward InsBegin chain (log)
    size_t logib_len = 0;
    uint32_t max_degree = 0;
    DevBuf gen_rec, gen_child_c, gen_init_c;  // sample_reads.hip: a 64-byte record of every node's child pick [N], the running
                                      // sums of the picks f64[E] and of the init pick f64[N]
};

// Successors for one segment length (run_succ.h with the segment as its run; seg_hull.h), on the device: what
// bwd_step's run skipping reads
struct RunSucc {
    int seg = 0;        // nodes per segment
    uint32_t nseg = 0;  // segments
    DevBuf off, ent;  // u32[nseg+1], u32[]
};

}  // namespace phmm

struct phmm_model {
    uint32_t N = 0, E = 0;
    phmm_params params{};
    phmm::LinParams lin{};
    std::vector<uint8_t> emission;
    std::vector<double> init_logp, trans_logp;
    std::vector<uint32_t> esrc, edst;
    // host CSR (petgraph order: newest edge first)
    std::vector<uint32_t> par_off, par_node, par_edge, chi_off, chi_node, chi_edge;
    std::vector<double> logib;  // forward InsBegin chain, log domain (forward.rs:541-545)
    phmm::ModelDev dev;
    // what phmm_sample_reads reads beside the CSR (dev.gen_*): built on its first call, dropped by model_upload
    bool gen_valid = false;
    double gen_init_total = 0.0;
    uint32_t gen_init_last = 0;
    double wf_ub_a = 0.0, wf_ub_b = 0.0;  // column total <= ub_a * max(m,i) + ub_b * p_ID * ib (model.cpp)
    // nodes of the descendant hop entries (bh) per node, kept on the host for the segment successors, and the
    // successors built so far, by segment length (the plans of one model use few); model_upload drops them
    std::vector<uint32_t> desc_off, desc_node;
    std::mutex rs_mu;
    std::vector<std::unique_ptr<phmm::RunSucc>> rs_cache;
    // Workspaces (DP tables, record pools, per-call scratch) belong to the DEVICE, not to the model: every
    // handle on a device shares one phmm::DevicePool, so a mapping model and a scoring model coexist
    // (multi_dbg/posterior.rs:247-255, 609-630) without each sizing its own tables from what is free.
    phmm::DevicePool *pool = nullptr;
    phmm::WorkSet &wset();
};

struct phmm_reads {
    uint64_t R = 0, total = 0;
    std::vector<uint8_t> bases;
    std::vector<uint64_t> off;
    uint64_t max_len = 0;
    // lazily uploaded device copies (per device of first use)
    mutable phmm::DevBuf d_bases, d_off;
    mutable bool on_device = false;
    // dense warm-up columns each read needed in the last adaptive-sparse call on this handle (empty: none
    // yet).  Only used to GROUP reads with similar warm-up lengths (results do not depend on the grouping):
    // a read group runs dense columns until its slowest read switches, and rows of 64 reads in which only a
    // few are still dense cost whole 64-byte sectors per live read.
    mutable std::vector<uint16_t> warm_hint;
    // what the last adaptive-sparse call did with each read (phmm_reads_last_call_info; diagnostics / parity tests):
    // PHMM_READ_* bits of include/phmm_amd.h
    mutable std::vector<uint32_t> last_flags;
};

struct phmm_mappings {
    uint64_t R = 0, total_pos = 0;
    std::vector<uint64_t> read_off;  // [R+1] position offsets per read
    std::vector<uint64_t> pos_off;   // [total_pos+1]
    std::vector<uint32_t> nodes;
    std::vector<double> logp;
    std::vector<uint32_t> read_max_list;  // [R] longest node list of each read
    std::vector<double> read_logp;        // [R] ln P(read) of the forward pass that produced the mappings (may be empty)
    std::vector<double> read_logp_backward;  // [R] ln B.tables[0].mb of the backward pass of the same call (may be empty)
    mutable phmm::DevBuf d_pos_off, d_nodes, d_logp;
    int device = -1;  // >= 0: the device whose pool takes the buffers back (phmm_mappings_destroy)
    mutable bool on_device = false;
    // Mappings produced by phmm_generate_mappings stay on the device (their next consumer is the
    // hinted forward kernel); the host vectors above are filled on first host access.
    mutable bool host_valid = true;
    uint64_t total_entries = 0;
    bool trusted = false;  // node ids come from our own kernels: no range check needed
};
namespace phmm {
void mappings_materialize_host(const phmm_mappings *mp);
}

// The alignment records of one phmm_run_with_mapping_alignments call (include/phmm_amd_align.h).  The arrays belong to
// the handle, not to the device workspace, and the handle borrows nothing.
struct phmm_alignments {
    uint64_t A = 0, total_ops = 0, total_runs = 0;
    int device = -1;
    phmm::DevBuf d_op_off, d_run_off;           // u64[A+1]
    phmm::DevBuf d_ops, d_run_node, d_run_len;  // u32[total_ops], u32[total_runs] twice (grown chunk by chunk)
};

// The sparse read-by-key matrix of one phmm_run_with_mapping_read_usage call (include/phmm_amd_usage.h), CSR over the
// reads.  The arrays belong to the handle, not to the device workspace, and the handle borrows nothing.
struct phmm_read_usage {
    uint64_t R = 0, K = 0, total = 0;
    int device = -1;
    phmm::DevBuf d_row_off;  // u64[R+1]
    phmm::DevBuf d_keys;     // u32[total]
    phmm::DevBuf d_usage;    // f64[total][3] (both grown chunk by chunk)
};

// The sparse read-by-key matrix of one phmm_run_with_mapping_read_edges call (include/phmm_amd_edges.h), CSR over the
// reads.  The arrays belong to the handle, not to the device workspace, and the handle borrows nothing.
struct phmm_read_edges {
    uint64_t R = 0, K = 0, total = 0;
    int device = -1;
    phmm::DevBuf d_row_off;  // u64[R+1]
    phmm::DevBuf d_keys;     // u32[total]
    phmm::DevBuf d_usage;    // f64[total]
};

// The sampler's state at one k (MultiDbg::to_likelihood, posterior.rs:247-255, through the greedy search of
// sample_posterior, posterior.rs:314-417): the current copy-number vector and every read's ln P under it, on the device.
// The value of read r under the current vector is val[r] + ln(T_at[r] / T): val[r] is what the kernels gave when r was
// last rescored and T_at[r] the (integer) T of that moment, so a read no move touches is rounded once however many
// moves lie between.  The arrays belong to the handle, not to the device workspace.
struct phmm_likelihood {
    phmm_model *m = nullptr;            // borrowed, as reads and mappings: they outlive the handle
    const phmm_reads *reads = nullptr;
    const phmm_mappings *mp = nullptr;
    uint32_t min_cn = 0;
    uint64_t T = 0;                     // sum of max(cn, min_cn) over the emittable nodes
    std::vector<uint32_t> cn;           // host mirror of d_cn (the O(changes) integer work reads it)
    phmm::DevBuf d_cn, d_val, d_tat;    // u32[N], f64[R], u64[R]
    std::vector<uint32_t> seen;         // [N] stamp of the change list that last named the node
    uint32_t stamp = 0;
    // Node groups (phmm_likelihood_set_groups): the k-mers of one compact edge, changed together.  Scoring in group
    // units reads g_cn / g_emit only, never cn[]; the mask tables of a group-form call have G + P words per 64
    // candidates, P = the distinct boundary parents over all groups (slot G + p).
    uint32_t G = 0, P = 0;
    std::vector<uint64_t> g_off;        // [G+1]
    std::vector<uint32_t> g_nodes;      // [g_off[G]]
    std::vector<uint32_t> g_of;         // [N] group of the node, PHMM_GROUP_MIXED (0xffffffff) for none
    std::vector<uint32_t> g_cn;         // [G] current copy number, PHMM_GROUP_MIXED once a node-form move split it
    std::vector<uint32_t> g_emit;       // [G] nodes with emission != 'n'
    std::vector<uint32_t> g_seen;       // [G] stamps, as `seen`
    std::vector<uint32_t> g_at;         // [G] scratch of a node-form move (index into its list of touched groups)
    uint32_t g_stamp = 0;
    // d_g_off u64[G+1], d_g_nodes u32[.], d_g_slot uint2[N] {group or none, boundary-parent slot or none},
    // d_bp_off u32[G+1], d_bp_slot u32[.] boundary-parent slots per group
    phmm::DevBuf d_g_off, d_g_nodes, d_g_slot, d_bp_off, d_bp_slot;
};

namespace phmm {

struct CallStats {
    double ms[5] = {0, 0, 0, 0, 0};
    uint64_t launches[5] = {0, 0, 0, 0, 0};
    uint64_t cells[5] = {0, 0, 0, 0, 0};
};
CallStats &stats();
bool timing_enabled();
// what the calling thread's last adaptive-sparse call shared by prefix (phmm_last_call_prefix_share): the columns J, 0 =
// off or declined, and the virtual lanes 4^J
struct ShareInfo {
    int J = 0;
    uint64_t lanes = 0;
};
ShareInfo &share_info();

// Per-launch HIP-event timing of one kernel class on the call's stream (bench.py's roofline):
// an event pair brackets every launch, the elapsed times are summed after one final sync.
struct LaunchTimer {
    bool on;
    std::vector<hipEvent_t> ev;
    explicit LaunchTimer(bool on_) : on(on_) {}
    ~LaunchTimer() {
        for (auto e : ev) (void)hipEventDestroy(e);
    }
    void begin() {
        if (!on) return;
        hipEvent_t e;
        HIP_CHECK(hipEventCreate(&e));
        HIP_CHECK(hipEventRecord(e, current_stream()));
        ev.push_back(e);
    }
    void end() { begin(); }
    double total_ms() {
        if (!on || ev.empty()) return 0.0;
        HIP_CHECK(hipEventSynchronize(ev.back()));
        double t = 0.0;
        for (size_t k = 0; k + 1 < ev.size(); k += 2) {
            float ms = 0;
            HIP_CHECK(hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
            t += ms;
        }
        return t;
    }
};

// PHMM_TRACE=1: print host-side phase times (syncs the stream; diagnostics only)
void trace(const char *tag);

// Developer knobs (environment variables; none is needed for normal use).  They are read in ONE place, when a compute
// entry point takes the device lock (api.cpp: guarded_on), never on the path of a call.
struct Knobs {
    bool trace = false;              // PHMM_TRACE: phase timings on stderr
    bool no_lean = false;            // PHMM_NO_LEAN: generic vector kernels instead of the one-lane-per-node ones
    bool no_wide_class = false;      // PHMM_NO_WIDE_CLASS: generic 400-slot kernels instead of the one-thread-per-node ones
    bool no_packed = false;          // PHMM_NO_PACKED: one candidate per wave
    int packed_cpl = 0;              // PHMM_PACKED_CPL: candidates per lane (0: automatic)
    bool no_exact_hinted = false;    // PHMM_NO_EXACT_HINTED: no wide-range pass over reads that a candidate cuts
    bool no_exact_dense = false;     // PHMM_NO_EXACT_DENSE: no log-domain pass over reads the dense certificate flags; their
                                     // scores come back NaN and their posteriors are left out (phmm_dense_tables ignores it)
    bool wide_hinted = false;        // PHMM_WIDE_HINTED (and PHMM_NO_WIDE_HINTED unset): mapping lists of 65-400 nodes on a block
                                     // (hinted_wide_kernel.h; the list pass: also wide_bwd_kernel.h).  Opt-in: DESIGN.md section 6
    bool no_wide_hinted = false;     // PHMM_NO_WIDE_HINTED: generic kernels for mapping lists of 65-400 nodes (hinted forward)
    bool no_wide_list_bwd = false;   // PHMM_NO_WIDE_LIST_BWD: with PHMM_WIDE_HINTED, the list backward of generate_mappings on carried
                                     // lists stays on the generic kernel (wide_bwd_kernel.h) -- the two halves apart, for tests
    bool wide_edge_bwd = false;      // PHMM_WIDE_EDGE_BWD: with PHMM_WIDE_HINTED, the backward half of run_with_mapping_edges on a block
                                     // as well (wide_backward_kernel<true, true>).  Opt-in of its own: DESIGN.md section 6
    bool wide_states_bwd = false;    // PHMM_WIDE_STATES_BWD: with PHMM_WIDE_HINTED, the backward half of run_with_mapping_states on a block
                                     // (wide_backward_kernel<true, false, BS, true>).  Opt-in of its own, as PHMM_WIDE_EDGE_BWD
    int wide_bwd_t = 0;              // PHMM_WIDE_BWD_T: threads of the list backward's block for reads with lists of at most 128 nodes,
                                     // 128 / 448 (anything else, 0: automatic -- 128 when there are more such reads than 448-thread
                                     // blocks the device holds at once, mapping_flow.hip)
    int wide_hinted_cpb = 0;         // PHMM_WIDE_HINTED_CPB: candidates per block of that class, 1 / 2 / 4 (anything else, 0: automatic)
    bool no_side_worker = false;     // PHMM_NO_SIDE_WORKER
    bool no_wide_handover = false;   // PHMM_NO_WIDE_HANDOVER
    int workers = 1;                 // PHMM_WORKERS: chunk pipeline
    int warm_cols = 0;               // PHMM_WARM_COLS: dense columns kept by the main plan (0: from N)
    int chunk_groups = 0;            // PHMM_CHUNK_GROUPS
    bool no_keep_all = false;        // PHMM_NO_KEEP_ALL: a small read set defers its slow reads too (see sparse_dyn.hip)
    int pipeline_min_groups = 8;     // PHMM_PIPELINE_MIN_GROUPS
    bool no_runmax = false;          // PHMM_NO_RUNMAX
    bool force_radix = false;        // PHMM_FORCE_RADIX
    bool serial_emit = false;        // PHMM_SERIAL_EMIT
    bool emit_high_priority = false; // PHMM_EMIT_HIGH_PRIORITY: list kernels of the dense head at the highest stream priority
    bool no_dma = false;             // PHMM_NO_DMA: forward rows through registers
    bool bwd_dma = false;            // PHMM_BWD_DMA
    bool no_bwd_skip = false;        // PHMM_NO_BWD_SKIP: the dense head's bwd_step computes every node run (no run masks)
    int dense_streams = 0;           // PHMM_DENSE_STREAMS
    int dense_w = 0;                 // PHMM_DENSE_W
    int dense_npt = 0;               // PHMM_DENSE_NPT
    double mem_fraction = 0.0;       // PHMM_MEM_FRACTION (0: the defaults, 0.9 tables / 0.95 planned)
    int share_prefix = -1;           // PHMM_SHARE_PREFIX: dense columns the reads of the main adaptive plan share by prefix
                                     // (-1, unset: the planner's choice; 0: off; 1..6: that many, where the plan is eligible)
};
const Knobs &knobs();
void refresh_knobs();

void model_build_host(phmm_model *m);    // CSR + logib
void model_upload(phmm_model *m);        // closures + device arrays
const RunSucc &model_run_successors(phmm_model *m, int seg);  // built and uploaded on first use of a segment length

// dense driver (dense.hip)
void run_dense(phmm_model *m, const phmm_reads *reads, double *out_lf, double *out_lb,
               double *out_nf);
// backward_sparse (backward.rs:146-185): sparse_bwd.hip
void full_prob_sparse_backward(phmm_model *m, const phmm_reads *reads, double *out_logp, double *out_total);
void backward_sparse_tables(phmm_model *m, const uint8_t *read, uint64_t len, double *b_m, double *b_i, double *b_d,
                            double *b_scal, uint8_t *is_dense);
void run_sparse(phmm_model *m, const phmm_reads *reads, double *out_lf, double *out_lb, double *out_nf);
void run_dense_edges(phmm_model *m, const phmm_reads *reads, double *out_lf, double *out_ef, double *out_if);
struct RecPool;
// sparse / hinted drivers (sparse.hip)
void full_prob_reads_hinted(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mp, uint32_t n_cand,
                            const double *init_logp, const double *trans_logp, double *out_logp,
                            double *out_total, const RecPool *pool = nullptr, const uint32_t *copy_nums = nullptr,
                            uint32_t min_copy_num = 0);
// the same loop over candidates given as changes to a base copy-number vector, rescoring only the reads they touch
void full_prob_reads_copy_num_changes(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mp,
                                      const uint32_t *base_cn, uint32_t min_cn, uint32_t n_cand, const uint64_t *chg_off,
                                      const uint32_t *chg_node, const uint32_t *chg_cn, double *out_logp,
                                      double *out_total, uint64_t *out_n_rescored);
// phmm_likelihood (sparse.hip): the same scoring against a vector and per-read values kept on the device
void likelihood_refresh(phmm_likelihood *lk);  // also the first scoring of phmm_likelihood_create
void likelihood_score_changes(phmm_likelihood *lk, uint32_t n_cand, const uint64_t *chg_off, const uint32_t *chg_node,
                              const uint32_t *chg_cn, double *out_logp, double *out_total, uint64_t *out_n_rescored,
                              bool by_group = false);  // by_group: chg_node holds group ids (phmm_likelihood_set_groups)
void likelihood_move(phmm_likelihood *lk, uint64_t n_chg, const uint32_t *chg_node, const uint32_t *chg_cn,
                     double *out_total, uint64_t *out_n_rescored, bool by_group = false);
void likelihood_current(const phmm_likelihood *lk, uint32_t *out_cn, double *out_logp, double *out_total);
void upload_reads(const phmm_reads *r);
void upload_mappings(const phmm_mappings *mp);
void mappings_map_nodes(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mp_in, const uint32_t *map_off,
                        const uint32_t *map_nodes, uint32_t n_old, phmm_mappings **out);
void generate_mappings_hinted(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mp_in, int use_max_ratio,
                              phmm_mappings **out, double *out_node_freq);
// run_with_mapping + to_edge_and_init_freqs over the reads (mapping_flow.hip)
void run_with_mapping_edges(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mp_in, double *out_lf,
                            double *out_ef, double *out_if);
void run_with_mapping_states(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mp_in, double *out_lf,
                             double *out_state_logp, uint32_t *out_best);
// The front half of the two edge calls (mapping_flow.hip): the edge-term list pass of every read and its records,
// compacted in position order.  The device arrays are workspace buffers; an EdgeScratchRelease in the caller gives them
// (and the caller's own sort buffers) back when the call ends.
struct EdgeRecords {
    std::vector<double> lf;             // [R] ln P of every read
    uint64_t total = 0;                 // records
    const uint32_t *key = nullptr;      // device [total]: the edge id, or E + v for Begin -> v
    const double *val = nullptr;        // device [total]
    const uint64_t *pos_off = nullptr;  // device [n_pos + 1]: the first record of every read position
    const double *logib = nullptr;      // device: the model's ib chain, logs
    const double *init = nullptr;       // device [N]
    const uint8_t *emis = nullptr;      // device [N]
};
struct EdgeScratchRelease {
    phmm_model *m;
    ~EdgeScratchRelease();
};
void edge_list_records(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mp_in, EdgeRecords &er);
// the two scalars of read r behind its Begin terms at its last base; logib: host copy of EdgeRecords::logib
void edge_end_terms(const phmm_model *m, const phmm_reads *reads, const std::vector<double> &lf,
                    const std::vector<double> &logib, uint64_t r, double &A_r, double &T_r);
// per read, how often it crossed every key (edge, Begin transition or a caller's group of them) (read_edges.hip);
// edge_key [E] / init_key [N]: the key or 0xffffffff, host arrays, nullptr with K == E + N = the default keys, else
// that kind left out; h == nullptr: scores and totals only
void run_with_mapping_read_edges(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mp, uint32_t K, bool mapped,
                                 const uint32_t *edge_key, const uint32_t *init_key, double *out_lf, double *out_end_terms,
                                 double *out_key_usage, phmm_read_edges *h);
void read_edges_export(const phmm_read_edges *u, uint64_t *row_off, uint32_t *keys, double *usage);
// A device consumer of the rows of the two calls below (alignments.hip).  With a sink every chunk's rows are staged in
// the workspace, as for a host out_path, and handed over on the call's stream behind the walk in place of the copy out.
struct RowSink {
    virtual ~RowSink() = default;
    // the reads r0 .. r1-1; row of base g in plane s: rows[(s * plane_rows + g - reads->off[r0]) * stride]
    virtual void chunk(uint64_t r0, uint64_t r1, const uint32_t *rows, uint64_t plane_rows, uint32_t stride) = 0;
};
// the best path of every read over its lists and its ln P (best_path.hip)
void run_with_mapping_best_path(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mp, double *out_logp,
                                uint32_t *out_path, uint32_t *out_counts, RowSink *sink = nullptr);
// the legal walk of the largest summed weight, the caller's weights per entry and kind (mea_path.hip), and the same walk
// on the posteriors of run_with_mapping_states, which stay on the device: the maximum-expected-accuracy path
void run_with_mapping_weighted_path(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mp, const double *weights,
                                    const double *ib_weight, double *out_score, uint32_t *out_path, uint32_t *out_counts,
                                    RowSink *sink = nullptr);
void run_with_mapping_mea_path(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mp, double del_weight,
                               double *out_lf, double *out_score, uint32_t *out_path, uint32_t *out_counts,
                               double *out_weights, RowSink *sink = nullptr);
// the forward and the backward table of every read over its lists, per entry and per base (list_tables.hip)
void run_with_mapping_tables(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mp, double *out_lf, double *out_lb,
                             double *out_f, double *out_fs, double *out_b, double *out_bs);
// n_samples draws from the posterior over paths of every read over its lists (sample_paths.hip)
void run_with_mapping_sample_paths(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mp, uint32_t n_samples,
                                   uint64_t seed, double *out_logp, double *out_path_logp, uint32_t *out_path,
                                   uint32_t *out_counts, uint32_t *out_node_usage, RowSink *sink = nullptr);
// the same paths as alignment records (alignments.hip); h == nullptr: scores and counts only
void run_with_mapping_alignments(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mp, uint32_t n_samples,
                                 uint64_t seed, double *out_logp, double *out_path_logp, uint32_t *out_counts,
                                 phmm_alignments *h);
void alignments_export(const phmm_alignments *h, uint64_t *op_off, uint32_t *ops, uint64_t *run_off, uint32_t *run_node,
                       uint32_t *run_len);
// per read, how often it used every key (node or node group) by state (read_usage.hip); key_of: [N] the key of the node
// or 0xffffffff, nullptr = the node itself; h == nullptr: scores and totals only
void run_with_mapping_read_usage(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mp, uint32_t K,
                                 const uint32_t *key_of, double *out_lf, double *out_key_usage, phmm_read_usage *h);
void read_usage_export(const phmm_read_usage *u, uint64_t *row_off, uint32_t *keys, double *usage);
// The keyed reduction behind the call above (read_usage.hip) with the two ends that depend on what a key is left to the
// caller: the states pass into the workspace plane, chunks of whole reads, the stable sort, the segments, the sums into
// the handle and the sort of the handle's keys behind the totals are the same for every key rule.
struct KeyedUsage {
    uint32_t K = 0;             // number of keys: a key is < K
    uint64_t fixed_bytes = 0;   // workspace the key builder holds beside the plane and the reads' first entries
    size_t totals_doubles = 0;  // length of the totals array
    const char *totals_name = "";
    // once, behind the states pass and the uploads of reads and lists: the key builder's own uploads
    std::function<void()> setup;
    // the sort keys of the n entries of the reads r0 .. r1-1, entry ent[r0] + i: keys[i] = (read - r0) << key_bits | key
    // (all ones: no key), vals[i] = i; ent: device, the first entry of every read
    std::function<void(hipStream_t s, const uint64_t *ent, uint32_t r0, uint32_t r1, uint32_t key_bits, uint32_t n,
                       uint64_t *keys, uint32_t *vals)>
        sort_keys;
    // the totals from the handle's T row entries stably sorted by key (sorted_rows: their index in usage[T][3])
    std::function<void(hipStream_t s, const uint32_t *sorted_keys, const uint32_t *sorted_rows, uint32_t T,
                       const double *usage, double *totals)>
        totals;
};
void run_with_mapping_keyed_usage(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mp, const KeyedUsage &ku,
                                  double *out_lf, double *out_totals, phmm_read_usage *h);
// per read and node, the posterior by state split by the read base there, and the per-node totals [N][9] (pileup.hip);
// h == nullptr: scores and totals only.  pileup_check_bases: PHMM_EINVAL for a read byte other than A C G T, host only.
void pileup_check_bases(const phmm_reads *reads);
void run_with_mapping_pileup(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mp, double *out_lf,
                             double *out_node_pileup, phmm_read_usage *h);
// reads drawn from the model, one walk per lane (sample_reads.hip)
void sample_reads(phmm_model *m, uint64_t first_index, uint64_t n_walks, uint32_t length, uint32_t length_kind,
                  const uint32_t *start_nodes, uint64_t n_start_nodes, uint64_t seed, uint8_t *out_bases, uint32_t *out_len,
                  uint32_t *out_flags, uint32_t *out_history, uint32_t history_cap, uint32_t *out_history_len,
                  uint32_t *out_node_usage);
struct MappingSink;
// by_ratio: use_max_ratio of forward_sparse (forward.rs:93-154); false = fixed warm-up + top n_active_nodes
void full_prob_reads_sparse(phmm_model *m, const phmm_reads *reads, double *out_logp, double *out_total,
                            MappingSink *sink, bool by_ratio = true, double *out_logb = nullptr);
void generate_mappings_sparse(phmm_model *m, const phmm_reads *reads, phmm_mappings **out, double *out_node_freq,
                              bool by_ratio = true);
void ensure_logib(phmm_model *m, size_t len);
void put_doubles(double *dst, const double *src_host, size_t n);
void put_bytes(void *dst, const void *src_host, size_t n);
void dense_tables(phmm_model *m, const uint8_t *read, uint64_t len, double *f_m, double *f_i,
                  double *f_d, double *f_scal, double *b_m, double *b_i, double *b_d,
                  double *b_scal);

}  // namespace phmm
