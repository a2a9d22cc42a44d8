// phmm_sample_reads: reads drawn from the model, one lane per walk (include/phmm_amd_generate.h writes out the walk, the
// random stream and the draw rule; tests/sample_reads_ref.py restates them).
//
// A step waits for the record of the node the previous step chose, and for nothing else: one 64-byte line per node
// (GenRec) holds the running sums of its child pick, the children and the children's emissions, so a step is one round
// trip to memory.  (A node of more than four children takes the pick through the CSR: offsets, sums, id, emission.)  No
// step computes an exp: the running sums of every node's child pick and of the init pick are built once per model on the
// host (gen_cache; sequential double adds in candidate order, as the rule states), and the weights of the state and
// emission decisions depend on the parameters alone -- lane 0 of a block builds their running sums into the LDS before
// the walks start.  The init pick binary-searches its sums.
//
// Stores: a lane packs 8 bases (4 history words) into registers and writes them with one 8-byte (16-byte) store into a
// staging row of the workspace whose stride is a multiple of that; per chunk one strided device copy brings the rows to
// the stride of the output, in place for a device destination and through a dense buffer and one plain copy for a host
// destination.  Under a workspace limit the walks run in chunks; walk i draws from the stream of i, so the chunks show
// nowhere.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "phmm_internal.h"

namespace phmm {

namespace {

constexpr uint64_t GEN_GOLD = 0x9E3779B97F4A7C15ull;
constexpr uint32_t GEN_M = 0, GEN_I = 1, GEN_D = 2, GEN_MB = 3, GEN_IB = 4, GEN_E = 5;  // state kinds of a walk

// The child pick of a node in one 64-byte line: candidate j (ascending edge index) has the running sum c[j], the child
// child[j] and that child's emission in byte j of emis; places from deg on repeat the last sum, so they are never chosen
// and c[3] is the total.  deg > GEN_REC_DEG: the node's pick goes through the CSR and child_c.
constexpr int GEN_REC_DEG = 4;
struct alignas(64) GenRec {
    double c[GEN_REC_DEG];
    uint32_t child[GEN_REC_DEG];
    uint32_t emis, deg;
    uint32_t pad[2];
};
static_assert(sizeof(GenRec) == 64, "one record per 64-byte line");

struct GenArgs {
    const uint32_t *chi_off, *chi_node;  // the model's child CSR (newest edge first)
    const uint8_t *emis;
    const GenRec *rec;                   // [n_nodes]
    const double *child_c;               // per node the running sums of its child pick, candidate j at chi_off[v] + j: nodes
                                         // of more than GEN_REC_DEG children
    const double *init_c;                // running sums of the init pick, [n_nodes]
    double init_total;
    uint32_t init_last, n_nodes;
    const uint32_t *start_nodes;         // custom start: ids and running sums, [n_start]
    const double *start_c;
    double start_total;
    uint32_t start_last, n_start;
    double p_match, p_mismatch, p_random, p_end;
    double p_MM, p_IM, p_DM, p_MI, p_II, p_DI, p_MD, p_ID, p_DD;
    uint64_t seed, index0;               // index of the chunk's first walk
    uint32_t n, length, kind, state_cap, history_cap;
    uint8_t *bases;                      // staging rows, bases_stride bytes each (a multiple of 8), zeroed
    uint32_t bases_stride;
    uint32_t *hist;                      // staging rows, hist_stride words each (a multiple of 4), all ones; or NULL
    uint32_t hist_stride;
    uint32_t *len, *flags, *hist_len;    // [n]
    uint32_t *usage;                     // [n_nodes] or NULL
    unsigned long long *cells;
};

__device__ __forceinline__ uint64_t gen_mix(uint64_t z) {  // the SplitMix64 finaliser
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ double gen_uniform(uint64_t x0, uint64_t d) {
    return (double)(gen_mix(x0 + d * GEN_GOLD) >> 11) * 0x1p-53;
}
__device__ __forceinline__ double gen_w(double t, double mx) { return t > -INFINITY ? exp(t - mx) : 0.0; }

// the smallest index with thr < c[index], else `last` (the last candidate of positive weight)
__device__ __forceinline__ uint32_t gen_search(const double *c, uint32_t n, double thr, uint32_t last) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (thr < c[mid]) hi = mid;
        else lo = mid + 1;
    }
    return lo < n ? lo : last;
}

// running sums of a decision with four candidates (a term of -inf: no candidate at that place); all zeros when no term
// is finite.  *last = the last candidate of positive weight
__device__ void gen_table(const double t0, const double t1, const double t2, const double t3, double *c, int *last) {
    const double t[4] = {t0, t1, t2, t3};
    double mx = -INFINITY;
    for (int i = 0; i < 4; i++) mx = fmax(mx, t[i]);
    double run = 0.0;
    *last = 0;
    for (int i = 0; i < 4; i++) {
        const double w = mx > -INFINITY ? gen_w(t[i], mx) : 0.0;
        run += w;
        c[i] = run;
        if (w > 0.0) *last = i;
    }
}

__global__ void __launch_bounds__(64) sample_reads_kernel(const GenArgs a) {
    __shared__ double s_c[5][4];  // by the state the step leaves: running sums of the next-state decision
    __shared__ int s_last[5];
    __shared__ double s_em[3];    // weights of a Match emission (the node's base, another base) and of an Ins emission
    if (threadIdx.x == 0) {
        const double pe = a.kind == PHMM_GEN_ENDABLE ? a.p_end : -INFINITY;
        gen_table(a.p_MM, a.p_MI, a.p_MD, pe, s_c[GEN_M], &s_last[GEN_M]);
        gen_table(a.p_IM, a.p_II, a.p_ID, pe, s_c[GEN_I], &s_last[GEN_I]);
        gen_table(a.p_DM, a.p_DI, a.p_DD, pe, s_c[GEN_D], &s_last[GEN_D]);
        gen_table(a.p_MI, a.p_MM, a.p_MD, -INFINITY, s_c[GEN_MB], &s_last[GEN_MB]);
        gen_table(a.p_II, a.p_IM, a.p_ID, -INFINITY, s_c[GEN_IB], &s_last[GEN_IB]);
        const double mx = fmax(a.p_match, a.p_mismatch);
        s_em[0] = mx > -INFINITY ? gen_w(a.p_match, mx) : 0.0;
        s_em[1] = mx > -INFINITY ? gen_w(a.p_mismatch, mx) : 0.0;
        s_em[2] = a.p_random > -INFINITY ? 1.0 : 0.0;
    }
    __syncthreads();
    const uint32_t w = blockIdx.x * 64u + threadIdx.x;
    if (w >= a.n) return;
    const uint64_t x0 = gen_mix(a.seed ^ gen_mix(a.index0 + w + GEN_GOLD));
    uint64_t d = 0;
    uint8_t *brow = a.bases + (size_t)w * a.bases_stride;
    uint32_t *hrow = a.hist ? a.hist + (size_t)w * a.hist_stride : nullptr;
    uint64_t bacc = 0;
    uint32_t nb = 0, hn = 0, n_state = 0, flags = 0;
    uint32_t h0 = PHMM_PATH_NONE, h1 = PHMM_PATH_NONE, h2 = PHMM_PATH_NONE, h3 = PHMM_PATH_NONE;

    auto push_base = [&](uint32_t b) {
        if (nb >= a.bases_stride) return;  // (never: a walk emits at most length + 1 bases)
        bacc |= (uint64_t)b << (8 * (nb & 7));
        nb++;
        if ((nb & 7) == 0) {
            *reinterpret_cast<uint64_t *>(brow + (nb - 8)) = bacc;
            bacc = 0;
        }
    };
    auto push_word = [&](uint32_t word) {
        h0 = h1, h1 = h2, h2 = h3, h3 = word;
        hn++;
        if (hrow && (hn & 3) == 0 && hn <= a.hist_stride) *reinterpret_cast<uint4 *>(hrow + (hn - 4)) = make_uint4(h0, h1, h2, h3);
    };
    auto enter = [&](uint32_t kind, uint32_t node) {  // the history word and the usage count of a state
        if (kind <= GEN_D) {
            push_word((node << 2) | kind);
            if (a.usage) atomicAdd(&a.usage[node], 1u);
        } else {
            push_word(kind == GEN_IB ? PHMM_PATH_INS_BEGIN : PHMM_GEN_END);
        }
    };
    // the emission of a Match on a node that emits `e` / of an Ins; false: no candidate of positive weight
    auto emit = [&](uint32_t kind, uint32_t e) {
        double w0, w1, w2, w3;
        if (kind == GEN_M) {
            const bool known = e == 'A' || e == 'C' || e == 'G' || e == 'T';
            const double wm = s_em[0], wx = known ? s_em[1] : (a.p_mismatch > -INFINITY ? 1.0 : 0.0);
            w0 = e == 'A' ? wm : wx, w1 = e == 'C' ? wm : wx, w2 = e == 'G' ? wm : wx, w3 = e == 'T' ? wm : wx;
        } else {
            w0 = w1 = w2 = w3 = s_em[2];
        }
        const double c0 = w0, c1 = c0 + w1, c2 = c1 + w2, c3 = c2 + w3;
        if (!(c3 > 0.0)) return false;
        const double thr = gen_uniform(x0, ++d) * c3;
        const int last = w3 > 0.0 ? 3 : w2 > 0.0 ? 2 : w1 > 0.0 ? 1 : 0;
        const int c = thr < c0 ? 0 : thr < c1 ? 1 : thr < c2 ? 2 : thr < c3 ? 3 : last;
        push_base(c == 0 ? 'A' : c == 1 ? 'C' : c == 2 ? 'G' : 'T');
        return true;
    };

    uint32_t kind = GEN_MB, node = 0;
    bool alive = true;
    if (a.n_start) {
        const double thr = gen_uniform(x0, ++d) * a.start_total;
        node = a.start_nodes[gen_search(a.start_c, a.n_start, thr, a.start_last)];
        kind = GEN_M;
        enter(GEN_M, node);
        if (!emit(GEN_M, a.emis[node])) {
            flags |= PHMM_GEN_DEAD_END;
            enter(GEN_E, 0);
            n_state++;
            alive = false;
        }
    }
    while (alive) {
        uint32_t nk = GEN_E, nn = 0, ne = 0;  // the next state, its node and that node's emission
        bool dead = false;
        if (kind <= GEN_D) {
            uint32_t child = 0, child_e = 0;
            const GenRec r = a.rec[node];
            if (r.deg <= (uint32_t)GEN_REC_DEG) {
                // 1. the child, from the node's record: one round trip for sums, ids and emissions
                const double q0 = r.c[0], q1 = r.c[1], q2 = r.c[2], q3 = r.c[3];
                if (!(q3 > 0.0)) dead = true;
                else {
                    const double thr = gen_uniform(x0, ++d) * q3;
                    const int last = q3 > q2 ? 3 : q2 > q1 ? 2 : q1 > q0 ? 1 : 0;
                    const int j = thr < q0 ? 0 : thr < q1 ? 1 : thr < q2 ? 2 : thr < q3 ? 3 : last;
                    child = j == 0 ? r.child[0] : j == 1 ? r.child[1] : j == 2 ? r.child[2] : r.child[3];
                    child_e = (r.emis >> (8 * j)) & 0xffu;
                }
            } else {
                // more children than a record holds: the same pick over the node's running sums in child_c; the CSR
                // lists the edges newest first, so candidate j is slot a1 - 1 - j
                const uint32_t a0 = a.chi_off[node], a1 = a.chi_off[node + 1];
                const double c_last = a.child_c[a1 - 1];
                if (!(c_last > 0.0)) dead = true;
                else {
                    const double thr = gen_uniform(x0, ++d) * c_last;
                    uint32_t pick = 0xffffffffu, last = 0;
                    double prev = 0.0;
                    for (uint32_t j = 0; j < a1 - a0; j++) {
                        const double c = a.child_c[a0 + j];
                        if (pick == 0xffffffffu && thr < c) pick = j;
                        if (c > prev) last = j;
                        prev = c;
                    }
                    child = a.chi_node[a1 - 1 - (pick != 0xffffffffu ? pick : last)];
                    child_e = a.emis[child];
                }
            }
            // 2. the next state
            const double c0 = s_c[kind][0], c1 = s_c[kind][1], c2 = s_c[kind][2], c3 = s_c[kind][3];
            if (!dead && !(c3 > 0.0)) dead = true;
            if (!dead) {
                const double thr = gen_uniform(x0, ++d) * c3;
                const int c = thr < c0 ? 0 : thr < c1 ? 1 : thr < c2 ? 2 : thr < c3 ? 3 : s_last[kind];
                nk = c == 0 ? GEN_M : c == 1 ? GEN_I : c == 2 ? GEN_D : GEN_E;
                nn = c == 1 ? node : child;
                ne = child_e;
            }
        } else {
            if (!(a.init_total > 0.0) || !(s_c[kind][3] > 0.0)) dead = true;
            else {
                const double thr = gen_uniform(x0, ++d) * a.init_total;
                const uint32_t v = gen_search(a.init_c, a.n_nodes, thr, a.init_last);
                const double c0 = s_c[kind][0], c1 = s_c[kind][1], c2 = s_c[kind][2];
                const double thr2 = gen_uniform(x0, ++d) * c2;
                const int c = thr2 < c0 ? 0 : thr2 < c1 ? 1 : thr2 < c2 ? 2 : s_last[kind];
                nk = c == 0 ? GEN_IB : c == 1 ? GEN_M : GEN_D;
                nn = v;
                ne = a.emis[v];
            }
        }
        if (dead) {
            flags |= PHMM_GEN_DEAD_END;
            enter(GEN_E, 0);
            n_state++;
            break;
        }
        enter(nk, nn);
        n_state++;
        if (nk == GEN_E) {
            flags |= PHMM_GEN_ENDED;
            break;
        }
        if ((nk == GEN_M || nk == GEN_I || nk == GEN_IB) && !emit(nk, ne)) {
            flags |= PHMM_GEN_DEAD_END;
            enter(GEN_E, 0);
            n_state++;
            break;
        }
        kind = nk;
        node = nn;
        if (a.kind == PHMM_GEN_EMIT_COUNT ? nb >= a.length : n_state >= a.length) break;
        if (n_state >= a.state_cap) {
            flags |= PHMM_GEN_STATE_CAP;
            break;
        }
    }
    if (nb & 7) *reinterpret_cast<uint64_t *>(brow + (nb & ~7u)) = bacc;
    const uint32_t hist_len = hn;
    if (hrow && (hn & 3) && (hn | 3u) < a.hist_stride) {
        while (hn & 3) push_word(PHMM_PATH_NONE);
    }
    if (a.history_cap && hist_len > a.history_cap) flags |= PHMM_GEN_HISTORY_TRUNCATED;
    a.len[w] = nb;
    a.flags[w] = flags;
    a.hist_len[w] = hist_len;
    atomicAdd(a.cells, (unsigned long long)n_state);
}

bool gen_is_device_pointer(const void *p) {
    hipPointerAttribute_t at;
    const bool dev = hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeDevice;
    if (!dev) (void)hipGetLastError();
    return dev;
}

struct GenTimer {  // device time of the whole call on its stream (index 2 of phmm_last_call_stats)
    hipEvent_t a = nullptr, b = nullptr;
    explicit GenTimer(bool on) {
        if (!on) return;
        HIP_CHECK(hipEventCreate(&a));
        HIP_CHECK(hipEventCreate(&b));
        HIP_CHECK(hipEventRecord(a, current_stream()));
    }
    ~GenTimer() {
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

// running sums of the draw rule over terms[order[0..n)] (order == NULL: 0..n-1), sequential double adds
// -> total; *last = the last candidate of positive weight
double gen_running_sums(const std::vector<double> &terms, const uint32_t *order, size_t n, std::vector<double> &c,
                        uint32_t *last) {
    double mx = -INFINITY;
    for (size_t i = 0; i < n; i++) mx = std::max(mx, terms[order ? order[i] : i]);
    c.assign(std::max<size_t>(n, 1), 0.0);
    *last = 0;
    double run = 0.0;
    for (size_t i = 0; i < n; i++) {
        const double t = terms[order ? order[i] : i];
        const double w = mx > -INFINITY && t > -INFINITY ? std::exp(t - mx) : 0.0;
        run += w;
        c[i] = run;
        if (w > 0.0) *last = (uint32_t)i;
    }
    return run;
}

// what the walks read of the model beside its CSR: built on first use, dropped by model_upload (set_probs, set_params)
void gen_cache(phmm_model *m) {
    if (m->gen_valid) return;
    std::vector<double> tl(std::max<size_t>(m->E, 1), 0.0), c;
    std::vector<GenRec> rec(m->N);
    for (uint32_t v = 0; v < m->N; v++) {  // candidate j of node v is the edge of CSR slot a1 - 1 - j: ascending edge index
        const uint32_t a0 = m->chi_off[v], a1 = m->chi_off[v + 1];
        double mx = -INFINITY, run = 0.0;
        for (uint32_t q = a0; q < a1; q++) mx = std::max(mx, m->trans_logp[m->chi_edge[q]]);
        for (uint32_t j = 0; j < a1 - a0; j++) {
            const double t = m->trans_logp[m->chi_edge[a1 - 1 - j]];
            run += mx > -INFINITY && t > -INFINITY ? std::exp(t - mx) : 0.0;
            tl[a0 + j] = run;
        }
        GenRec r{};
        r.deg = a1 - a0;
        for (uint32_t j = 0; j < (uint32_t)GEN_REC_DEG && r.deg <= (uint32_t)GEN_REC_DEG; j++) {
            r.c[j] = j < r.deg ? tl[a0 + j] : run;
            if (j < r.deg) {
                r.child[j] = m->chi_node[a1 - 1 - j];
                r.emis |= (uint32_t)m->emission[r.child[j]] << (8 * j);
            }
        }
        rec[v] = r;
    }
    m->gen_init_total = gen_running_sums(m->init_logp, nullptr, m->N, c, &m->gen_init_last);
    m->dev.gen_child_c.upload(tl.data(), sizeof(double) * tl.size());
    m->dev.gen_rec.upload(rec.data(), sizeof(GenRec) * rec.size());
    m->dev.gen_init_c.upload(c.data(), sizeof(double) * c.size());
    HIP_CHECK(hipStreamSynchronize(current_stream()));
    m->gen_valid = true;
}

}  // namespace

void sample_reads(phmm_model *m, uint64_t first_index, uint64_t n_walks, uint32_t length, uint32_t length_kind,
                  const uint32_t *start_nodes, uint64_t n_start_nodes, uint64_t seed, uint8_t *out_bases, uint32_t *out_len,
                  uint32_t *out_flags, uint32_t *out_history, uint32_t history_cap, uint32_t *out_history_len,
                  uint32_t *out_node_usage) {
    hipStream_t s = current_stream();
    CallStats &st = stats();
    st = CallStats();
    const uint32_t N = m->N;
    gen_cache(m);
    GenTimer tm(timing_enabled());
    WorkSet &ws = m->wset();
    DevBuf &ctl = ws.aux[3], &brows = ws.aux[1], &hrows = ws.aux[5], &usage = ws.aux[6], &starts = ws.aux[7],
           &bdense = ws.aux[8], &hdense = ws.aux[9];

    GenArgs a{};
    a.chi_off = m->dev.chi_off.as<uint32_t>();
    a.chi_node = m->dev.chi_node.as<uint32_t>();
    a.emis = m->dev.emis.as<uint8_t>();
    a.child_c = m->dev.gen_child_c.as<double>();
    a.rec = m->dev.gen_rec.as<GenRec>();
    a.init_c = m->dev.gen_init_c.as<double>();
    a.init_total = m->gen_init_total;
    a.init_last = m->gen_init_last;
    a.n_nodes = N;
    const phmm_params &pp = m->params;
    a.p_match = pp.p_match, a.p_mismatch = pp.p_mismatch, a.p_random = pp.p_random, a.p_end = pp.p_end;
    a.p_MM = pp.p_MM, a.p_IM = pp.p_IM, a.p_DM = pp.p_DM, a.p_MI = pp.p_MI, a.p_II = pp.p_II, a.p_DI = pp.p_DI;
    a.p_MD = pp.p_MD, a.p_ID = pp.p_ID, a.p_DD = pp.p_DD;
    a.seed = seed;
    a.length = length;
    a.kind = length_kind;
    a.state_cap = 8u * length + 64u;
    a.history_cap = history_cap;
    a.bases_stride = (length + 1 + 7) / 8 * 8;
    a.hist_stride = out_history ? (uint32_t)(((uint64_t)history_cap + 3) / 4 * 4) : 0;

    // the start nodes and their running sums, in the order given
    if (n_start_nodes) {
        std::vector<double> c;
        const double total = gen_running_sums(m->init_logp, start_nodes, n_start_nodes, c, &a.start_last);
        const size_t cbytes = sizeof(double) * n_start_nodes;
        starts.reserve(cbytes + sizeof(uint32_t) * n_start_nodes);
        HIP_CHECK(hipMemcpyAsync(starts.p, c.data(), cbytes, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(starts.as<char>() + cbytes, start_nodes, sizeof(uint32_t) * n_start_nodes,
                                 hipMemcpyHostToDevice, s));
        HIP_CHECK(hipStreamSynchronize(s));  // (c dies at the end of this block)
        a.start_c = starts.as<double>();
        a.start_nodes = (const uint32_t *)(starts.as<char>() + cbytes);
        a.start_total = total;
        a.n_start = (uint32_t)n_start_nodes;
    }

    // the usage counts: cleared here, added into by the walks (a device out_node_usage is written in place)
    const bool usage_in_place = out_node_usage && gen_is_device_pointer(out_node_usage);
    if (out_node_usage) {
        if (!usage_in_place) usage.reserve(sizeof(uint32_t) * N);
        a.usage = usage_in_place ? out_node_usage : usage.as<uint32_t>();
        HIP_CHECK(hipMemsetAsync(a.usage, 0, sizeof(uint32_t) * N, s));
    }

    // chunks of consecutive walks whose staging rows and per-walk words fit the budget
    // (a host destination gets its rows through a dense device copy: a strided copy to pageable host memory goes row by row)
    const bool dense_bases = out_bases && !gen_is_device_pointer(out_bases),
               dense_hist = out_history && !gen_is_device_pointer(out_history);
    const uint64_t per_walk = (uint64_t)a.bases_stride + sizeof(uint32_t) * a.hist_stride + 3 * sizeof(uint32_t) +
                              (dense_bases ? (uint64_t)length + 1 : 0) + (dense_hist ? sizeof(uint32_t) * (uint64_t)history_cap : 0);
    const uint64_t fixed = 256 + (out_node_usage && !usage_in_place ? sizeof(uint32_t) * (uint64_t)N : 0),
                   limit = table_budget(*m->pool);
    const uint64_t budget = limit > fixed ? limit - fixed : 0;
    const uint64_t chunk = std::max<uint64_t>(1, std::min<uint64_t>({n_walks, budget / per_walk, (uint64_t)1 << 30}));
    ctl.reserve(256 + 3 * sizeof(uint32_t) * chunk);
    brows.reserve(chunk * a.bases_stride);
    if (a.hist_stride) hrows.reserve(sizeof(uint32_t) * chunk * a.hist_stride);
    if (dense_bases) bdense.reserve(chunk * ((uint64_t)length + 1));
    if (dense_hist) hdense.reserve(sizeof(uint32_t) * chunk * history_cap);
    a.cells = ctl.as<unsigned long long>();
    a.len = (uint32_t *)(ctl.as<char>() + 256);
    a.flags = a.len + chunk;
    a.hist_len = a.flags + chunk;
    a.bases = brows.as<uint8_t>();
    a.hist = a.hist_stride ? hrows.as<uint32_t>() : nullptr;
    HIP_CHECK(hipMemsetAsync(a.cells, 0, sizeof(unsigned long long), s));
    trace("sample reads setup");
    for (uint64_t w0 = 0; w0 < n_walks; w0 += chunk) {
        const uint64_t n = std::min(chunk, n_walks - w0);
        a.index0 = first_index + w0;
        a.n = (uint32_t)n;
        HIP_CHECK(hipMemsetAsync(a.bases, 0, n * a.bases_stride, s));
        if (a.hist) HIP_CHECK(hipMemsetAsync(a.hist, 0xff, sizeof(uint32_t) * n * a.hist_stride, s));
        hipLaunchKernelGGL(sample_reads_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, a);
        HIP_CHECK(hipGetLastError());
        st.launches[2]++;
        if (out_bases) {
            const size_t row = (size_t)length + 1;
            uint8_t *dst = out_bases + w0 * row;
            HIP_CHECK(hipMemcpy2DAsync(dense_bases ? bdense.p : dst, row, a.bases, a.bases_stride, row, n,
                                       hipMemcpyDeviceToDevice, s));
            if (dense_bases) HIP_CHECK(hipMemcpyAsync(dst, bdense.p, row * n, hipMemcpyDeviceToHost, s));
        }
        if (out_history) {
            const size_t row = sizeof(uint32_t) * history_cap;
            uint32_t *dst = out_history + w0 * history_cap;
            HIP_CHECK(hipMemcpy2DAsync(dense_hist ? hdense.p : dst, row, a.hist, sizeof(uint32_t) * a.hist_stride, row, n,
                                       hipMemcpyDeviceToDevice, s));
            if (dense_hist) HIP_CHECK(hipMemcpyAsync(dst, hdense.p, row * n, hipMemcpyDeviceToHost, s));
        }
        HIP_CHECK(hipStreamSynchronize(s));
        if (out_len) copy_out(out_len + w0, a.len, sizeof(uint32_t) * n);
        if (out_flags) copy_out(out_flags + w0, a.flags, sizeof(uint32_t) * n);
        if (out_history_len) copy_out(out_history_len + w0, a.hist_len, sizeof(uint32_t) * n);
        trace("sample reads chunk");
    }
    st.ms[2] += tm.stop();
    unsigned long long cells = 0;
    HIP_CHECK(hipMemcpy(&cells, a.cells, sizeof cells, hipMemcpyDeviceToHost));
    st.cells[2] = cells;
    if (out_node_usage && !usage_in_place) copy_out(out_node_usage, a.usage, sizeof(uint32_t) * N);
    trace("sample reads outputs");
}

}  // namespace phmm
