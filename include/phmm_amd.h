/*
 * phmm_amd.h -- C ABI of the MI355X-native profile-HMM read-likelihood path.
 *
 * Drop-in boundary for dbgphmm's `src/hmmv2`: the reference has no FFI layer; its
 * boundary is the set of `impl PHMMModel` methods.  Each entry point below names the
 * reference method it replaces (file:line relative to the dbgphmm source tree).  A Rust
 * shim flattens its petgraph `PHMMModel` into these arrays and calls through
 * `extern "C"` (INTEGRATION.md shows the binding).
 *
 * Conventions
 *  - plain pointers and sizes only; all probabilities cross the boundary as f64
 *    natural-log values (the reference's `Prob`), node ids as u32 (`NodeIndex`),
 *    bases as ASCII u8.
 *  - input pointers are HOST pointers.  Output pointers may be host OR device
 *    pointers (detected with hipPointerGetAttributes): device outputs let the caller
 *    all-reduce `node_freq` / totals over RCCL without a host round trip.
 *    Where the text of an entry point says "host pointer" for an output (phmm_likelihood_current's copy_nums,
 *    phmm_mappings_export, the single-read table dumps, phmm_q_score_exact) it is written with a plain host copy.
 *  - streams: phmm_set_stream() is a per-thread setting.  All device work of a call -- its kernels, the worker
 *    and side streams it uses inside, the copies into device outputs -- is ordered after everything the thread's
 *    stream held when the call was made, and when the call returns every output is complete ON THAT STREAM:
 *    work queued on it afterwards, or anything behind a hipStreamSynchronize of it, sees the results.  (As built
 *    today every compute entry point also synchronises the stream before it returns, because it reads error
 *    words and totals back; a caller should rely on the stream order only.)  Nothing is ordered against other
 *    streams, the NULL stream included, when the caller's stream is hipStreamNonBlocking.
 *  - every function returns 0 on success or a negative PHMM_E* code;
 *    phmm_last_error() returns the message (thread-local).  Nothing unwinds across
 *    the ABI.  Where the reference panics (empty read, capacity overflow) the call
 *    fails with PHMM_EINVAL / PHMM_ECAPACITY.
 *  - handles own their model / read / mapping arrays; destroy them explicitly.  The DP
 *    workspaces belong to the device (phmm_release_workspace).  Compute calls on one
 *    device are serialised internally; the natural cut is one call per read set (all
 *    reads x all candidates), replacing the rayon `par_iter` loops of the reference.
 */
#ifndef PHMM_AMD_H
#define PHMM_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PHMM_OK 0
#define PHMM_EINVAL (-1)    /* bad argument (reference: assert!/panic!) */
#define PHMM_ENODEVICE (-2) /* no usable MI355X / HIP runtime error */
#define PHMM_ENOMEM (-3)    /* device or host allocation failed */
#define PHMM_ECAPACITY (-4) /* >400 active nodes (reference: ArrayVec panic, table.rs:22) */
#define PHMM_EINTERNAL (-5)

#define PHMM_MAX_ACTIVE_NODES 400 /* src/hmmv2/table.rs:22 */
#define PHMM_MAX_GAPS 6           /* supported upper bound of n_max_gaps (reference default 4) */

/* PHMMParams, src/hmmv2/params.rs:16-66.  p_* are natural-log probabilities. */
typedef struct phmm_params {
    double p_mismatch, p_match, p_random, p_gap_open, p_gap_ext, p_end;
    double p_MM, p_IM, p_DM, p_MI, p_II, p_DI, p_MD, p_ID, p_DD;
    int64_t n_active_nodes;
    double active_node_max_ratio;
    int64_t n_warmup;
    int64_t warmup_threshold;
    int64_t n_max_gaps;
} phmm_params;

typedef struct phmm_model phmm_model;       /* PHMMModel<N,E>, src/hmmv2/common.rs:61-64 */
typedef struct phmm_reads phmm_reads;       /* ReadCollection<S>, src/common/collection.rs:38-83 */
typedef struct phmm_mappings phmm_mappings; /* Mappings, src/hmmv2/hint.rs:150-152 */

/* thread-local message of the last failing call */
const char *phmm_last_error(void);
/* "dbgphmm_amd <version> gfx950" */
const char *phmm_version(void);
/* number of visible HIP devices (0 without a GPU); does not initialise a context */
int phmm_device_count(void);
/* select the device for this thread's subsequent calls (one process per GPU: LOCAL_RANK) */
int phmm_set_device(int device);
/* run subsequent work of this thread on the given hipStream_t (NULL = default stream).  Per thread: a thread that
 * never called it is on the NULL stream whatever other threads hold, and the setting stays until the thread sets
 * another.  The stream must outlive the calls made on it; see "streams" in the conventions above for the ordering a
 * call keeps.  The workspaces belong to the device, not to the stream: calls on different streams are serialised and
 * each leaves nothing running on the workspaces when it returns. */
int phmm_set_stream(void *hip_stream);
/* upper bound (bytes) for the workspace of one call; 0 = automatic: the adaptive flow plans 95 % of (free + already
 * held) HBM for ALL its buffers, the dense drivers take 90 % for their tables */
int phmm_set_workspace_limit(uint64_t bytes);
/* Workspaces (DP tables, record pools, scratch) belong to the DEVICE and are shared by every handle on it:
 * a mapping model and a scoring model can be alive together, as in multi_dbg/posterior.rs:247-255, 609-630
 * (the reference builds a fresh PModel per call and drops its tables on return).  They grow on demand and are
 * kept between calls; so are the device arrays of destroyed phmm_mappings (up to 6 buffers / 8 GB: the next
 * phmm_generate_mappings call takes them instead of allocating).  phmm_release_workspace() returns all of it to the
 * device (the calling thread's current device must be idle), phmm_workspace_bytes() says how much is held.  Calls that compute on one device are
 * serialised inside the library whatever handle or thread they come from. */
int phmm_release_workspace(void);
uint64_t phmm_workspace_bytes(void);

/* PHMMParams::new / uniform, params.rs:73-125 (arguments are LINEAR probabilities) */
int phmm_params_new(double p_mismatch, double p_gap_open, double p_gap_ext, double p_end,
                    int64_t n_active_nodes, int64_t n_warmup, phmm_params *out);
int phmm_params_uniform(double p, phmm_params *out);

/* ---- model ------------------------------------------------------------------
 * Replaces SeqGraph::to_phmm's output (src/graph/seq_graph.rs:213-223): a PModel
 * flattened to arrays.  Edges in petgraph insertion order.  The topology stays on the
 * device; phmm_model_set_probs swaps init/trans for the next candidate copy-number
 * vector (what `dbg.clone(); set_copy_nums; to_phmm` does per candidate,
 * src/multi_dbg/posterior.rs:483-501). */
int phmm_model_create(uint32_t n_nodes, uint32_t n_edges, const uint8_t *emission,
                      const double *init_logp, const uint32_t *edge_src,
                      const uint32_t *edge_dst, const double *trans_logp,
                      const phmm_params *params, phmm_model **out);
int phmm_model_set_probs(phmm_model *m, const double *init_logp, const double *trans_logp);
int phmm_model_set_params(phmm_model *m, const phmm_params *params);
uint32_t phmm_model_n_nodes(const phmm_model *m);
uint32_t phmm_model_n_edges(const phmm_model *m);
void phmm_model_destroy(phmm_model *m);

/* ---- reads ------------------------------------------------------------------
 * bases: concatenated reads; offsets[R+1].  Empty reads are rejected (the reference
 * panics in last_table(), table.rs:388). */
int phmm_reads_create(const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads,
                      phmm_reads **out);
uint64_t phmm_reads_count(const phmm_reads *r);
uint64_t phmm_reads_total_bases(const phmm_reads *r);
void phmm_reads_destroy(phmm_reads *r);
/* What the most recent adaptive-sparse call on these reads (phmm_generate_mappings / phmm_full_prob_reads with
 * mappings == NULL and use_max_ratio != 0) did with each read -- for tools and parity tests that want to sample
 * the rare code paths.  out_dense_columns[R]: the read's dense/sparse switch position = number of dense warm-up
 * tables (forward.rs:107-137; the read length when it never switched).  out_flags[R]: PHMM_READ_* bits.
 * Either may be NULL.  PHMM_EINVAL before the first such call. */
#define PHMM_READ_DEFERRED 1u      /* still dense after the main plan's kept columns: redone in the all-columns plan */
#define PHMM_READ_WIDE_FRONTIER 2u /* its frontier outgrew the one-lane-per-node class at least once (400-slot bursts) */
#define PHMM_READ_FORCED_SWITCH 4u /* switched at n_warmup with more than 400 nodes inside the ratio (top-400 selection) */
int phmm_reads_last_call_info(const phmm_reads *r, uint16_t *out_dense_columns, uint32_t *out_flags);

/* ---- dense forward + backward + posteriors ----------------------------------
 * PHMMModel::run over a read set (src/hmmv2/freq.rs:42-46) followed by
 * PHMMOutput::{to_full_prob_forward, to_full_prob_backward, to_node_freqs}
 * (table.rs:482-494; freq.rs:245-255), i.e. PHMMModel::to_node_freqs /
 * to_full_prob_parallel (freq.rs:89-119) in one call.
 *   out_logp_forward[R]  = ln P(read) from the last forward table's `e`
 *   out_logp_backward[R] = ln P(read) from the first backward table's `mb`   (may be NULL)
 *   out_node_freq[N]     = sum over reads of node usage posteriors          (may be NULL)
 * Any output may be a device pointer. */
int phmm_run_dense(phmm_model *m, const phmm_reads *reads, double *out_logp_forward,
                   double *out_logp_backward, double *out_node_freq);

/* Transition posteriors: PHMMOutput::to_edge_and_init_freqs (freq.rs:276-298, 332-389) of a dense
 * `run`, summed over the reads (EM-style uses / tests; not called by `infer`).
 *   out_edge_freq[E] = sum over reads, positions and the six transition kinds (mm im dm md id dd) of
 *                      P(edge used | read);  out_init_freq[N] = the same for Begin -> node (mm im md id).
 * Any output may be NULL or a device pointer.  Keeps the full backward tables of a chunk in HBM. */
int phmm_run_dense_edges(phmm_model *m, const phmm_reads *reads, double *out_logp_forward,
                         double *out_edge_freq, double *out_init_freq);

/* Q function of an EM step from those posteriors: q_score_exact (src/hmmv2/q.rs:66-96).
 *   out_q[0] = init  = sum over emittable v of init_freq[v] * ln init_prob(v)
 *   out_q[1] = trans = sum over edges v -> w between emittable nodes of edge_freq[e] * ln trans_prob(e)
 *   out_q[2] = prior = 0 (q.rs:94-95);  QScore::total() is the sum of the three (q.rs:30-36).
 * Folded in the reference's order (nodes by id, the children of a node newest edge first).  A -inf
 * init / trans probability on that walk is PHMM_EINVAL (the reference asserts is_finite, q.rs:79, 88).
 * Host pointers; O(N + E) on the host from the probabilities the model was created / last set with. */
int phmm_q_score_exact(const phmm_model *m, const double *edge_freq, const double *init_freq,
                       double *out_q);

/* Dense tables of ONE read for parity tests / `inspect`-style tools:
 * PHMMModel::forward / backward (forward.rs:24-45; backward.rs:24-53).
 * f_m/f_i/f_d: [L][N] natural-log values of F.tables[i]; f_scal: [L][3] = mb, ib, e.
 * b_*: the same for B.tables[i].  Any pointer may be NULL.  Host pointers. */
int phmm_dense_tables(phmm_model *m, const uint8_t *read, uint64_t len, double *f_m,
                      double *f_i, double *f_d, double *f_scal, double *b_m, double *b_i,
                      double *b_d, double *b_scal);

/* ---- mappings (hints) ---------------------------------------------------------
 * Mappings (hint.rs:27-30,150-152) as a 3-level CSR over the reads of `reads`:
 * pos_off[total_bases+1] indexes nodes[]/logp[] for every read position in read order. */
int phmm_mappings_create(const phmm_reads *reads, const uint64_t *pos_off,
                         const uint32_t *nodes, const double *logp, phmm_mappings **out);
uint64_t phmm_mappings_total_positions(const phmm_mappings *mp);
uint64_t phmm_mappings_total_entries(const phmm_mappings *mp);
int phmm_mappings_export(const phmm_mappings *mp, uint64_t *pos_off, uint32_t *nodes,
                         double *logp);
/* Mappings::to_node_freqs, hint.rs:161-171 */
int phmm_mappings_node_freqs(const phmm_mappings *mp, uint32_t n_nodes, double *out_freq);
/* ln P(read) (forward `e` of the last table, table.rs:395-401) of the run_sparse_adaptive pass
 * that produced `mp` in phmm_generate_mappings: PHMMOutput::to_full_prob_forward per read.
 * out_logp[R] / out_total (their sum) may be NULL or device pointers. */
int phmm_mappings_read_logp(const phmm_mappings *mp, double *out_logp, double *out_total);
/* ln P(read) of the backward pass of the same call: B.tables[0].mb, PHMMOutput::to_full_prob_backward per read
 * (table.rs:492-494) -- backward_by_forward (backward.rs:101-142) without input mappings, backward_with_mapping
 * (backward.rs:59-90) with them; begin states as in backward.rs:499-555.  Equal to phmm_mappings_read_logp up to
 * the mass the truncated frontier lost: the gap is the reference's own self-check of a read.
 * out_logp[R] / out_total (their sum) may be NULL or device pointers.  PHMM_EINVAL for mappings not produced by
 * phmm_generate_mappings (phmm_mappings_map_nodes carries the values over). */
int phmm_mappings_read_logp_backward(const phmm_mappings *mp, double *out_logp, double *out_total);
void phmm_mappings_destroy(phmm_mappings *mp);

/* ---- read-set likelihood ------------------------------------------------------
 * PHMMModel::to_full_prob_reads (freq.rs:175-192): per read
 * forward_with_mapping_score_only (forward.rs:79-89) when mappings != NULL, else
 * forward_sparse_score_only(use_max_ratio) (forward.rs:158-206).
 *   out_logp[R] per-read ln P; out_total = their sum (rayon `.product()`).
 * Either may be NULL / a device pointer.
 * With mappings, a read whose listed nodes all die under the model (a k-mer on its path at copy
 * number 0) still gets the reference's finite ln P: the InsBegin chain re-enters the graph behind the
 * cut (forward.rs:337-359, 541-545); -inf only where the reference's own value is -inf. */
int phmm_full_prob_reads(phmm_model *m, const phmm_reads *reads,
                         const phmm_mappings *mappings, int use_max_ratio,
                         double *out_logp, double *out_total);

/* Candidate-batched form of the loop in sample_posterior_once
 * (src/multi_dbg/posterior.rs:483-515): C candidate (init, trans) vectors on one
 * topology, all reads, hinted forward.  init_logp [C][N], trans_logp [C][E] host
 * pointers; out_logp [C][R] (may be NULL), out_total [C]. */
int phmm_full_prob_reads_candidates(phmm_model *m, const phmm_reads *reads,
                                    const phmm_mappings *mappings, uint32_t n_candidates,
                                    const double *init_logp, const double *trans_logp,
                                    double *out_logp, double *out_total);

/* The same loop with the candidates given as COPY-NUMBER vectors (what the sampler actually
 * varies: `dbg.set_copy_nums(copy_nums); dbg.to_phmm(param)`, posterior.rs:485-487, 253) instead of
 * probability vectors: copy_nums [C][N] (host pointer; PHMM node v = DBG k-mer v), and init / trans
 * are derived on the device as SeqGraph::to_phmm does (seq_graph.rs:110-135, 160-209, no edge copy
 * numbers): init[v] = max(cn[v], min_copy_num) / sum over emittable nodes, trans[v->w] =
 * max(cn[w], min_copy_num) / sum over the emittable children of v; 0 into / from a non-emittable
 * node (emission 'n').  min_copy_num: 0 = to_phmm, 1 = to_non_zero_phmm (seq_graph.rs:263-273).
 * Removes the per-candidate host rebuild and the C x (N + E) x 8-byte upload of the form above. */
int phmm_full_prob_reads_copy_nums(phmm_model *m, const phmm_reads *reads,
                                   const phmm_mappings *mappings, uint32_t n_candidates,
                                   const uint32_t *copy_nums, uint32_t min_copy_num,
                                   double *out_logp, double *out_total);

/* The same loop with each candidate given as changes to a base copy-number vector, rescoring only the reads it
 * touches.  Candidate c = base_copy_nums[N] with cn[change_node[j]] = change_copy_num[j] (absolute new values) for
 * j in [change_off[c], change_off[c+1]); change_off has n_candidates + 1 entries.  All inputs are host pointers.
 * With e(v) = max(cn[v], min_copy_num), T = sum of e over the emittable nodes, D_c = the nodes whose e differs from the
 * base and A_c = D_c plus their parents: a read none of whose listed nodes is in A_c gets ln P_base + ln(T_base / T_c)
 * (exact in real arithmetic: every init it reads is scaled by T_base / T_c and no trans it uses changes); the others
 * are run through the kernels.  A candidate with T_c = 0, or every candidate when T_base = 0, is scored in full.
 *   out_logp [C][R], out_total [C]: as phmm_full_prob_reads_copy_nums on the materialised vectors (rescored reads
 *   bit-equal to it, the others within rounding);  out_n_rescored [C]: non-empty reads run through the kernels.
 * Any output may be NULL or a device pointer.  NULL mappings or base, mappings of another read set, change_off not
 * starting at 0 or decreasing, a node id >= N, a node listed twice within one candidate and node degree > 8 are
 * PHMM_EINVAL, with nothing written; n_candidates = 0 writes nothing.  Repeated calls return the same bits. */
int phmm_full_prob_reads_copy_num_changes(phmm_model *m, const phmm_reads *reads,
        const phmm_mappings *mappings, const uint32_t *base_copy_nums, uint32_t min_copy_num,
        uint32_t n_candidates, const uint64_t *change_off, const uint32_t *change_node,
        const uint32_t *change_copy_num, double *out_logp, double *out_total, uint64_t *out_n_rescored);

/* ---- the sampler's state on the device -------------------------------------------
 * MultiDbg::to_likelihood (multi_dbg/posterior.rs:247-255) through the greedy search of sample_posterior
 * (posterior.rs:314-417): score every neighbour of the current copy-number vector (sample_posterior_once,
 * posterior.rs:470-528), move to the best one or to the union of several independent moves (posterior.rs:532-590),
 * repeat from there.  The handle keeps the current vector and every read's ln P under it on the device for the whole
 * search at one k: candidates are scored against them with no base pass and no upload of the vector, and a move
 * rescores only the reads it touches.
 * The handle BORROWS model, reads and mappings: they must outlive it.  Its own arrays belong to the handle, not to
 * the device workspace (phmm_release_workspace between two calls changes no result).  Every call takes the device
 * lock.  A call that fails (PHMM_EINVAL for what phmm_full_prob_reads_copy_num_changes refuses, or any other error)
 * writes no output and leaves the vector, T and the per-read values as they were.  phmm_model_set_probs does not
 * concern the handle (init / trans come from copy numbers); after phmm_model_set_params call phmm_likelihood_refresh. */
typedef struct phmm_likelihood phmm_likelihood;

/* Scores copy_nums[N] (host) in full once -- phmm_full_prob_reads_copy_nums with one candidate -- and keeps the
 * vector, T = sum of max(cn, min_copy_num) over the emittable nodes, and every read's ln P under it. */
int phmm_likelihood_create(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mappings,
                           const uint32_t *copy_nums, uint32_t min_copy_num, phmm_likelihood **out);

/* C candidates as changes to the CURRENT vector (the CSR of phmm_full_prob_reads_copy_num_changes, host pointers).
 * Returns what that call returns with the current vector as its base: the same reads rescored per candidate, rescored
 * (read, candidate) pairs bit-equal to phmm_full_prob_reads_copy_nums on the materialised vector, every other pair
 * ln P_current + ln(T / T_c).  out_logp [C][R] / out_total [C] / out_n_rescored [C]: NULL, host or device; with
 * out_logp == NULL no [C][R] matrix is formed.  n_candidates = 0 writes nothing. */
int phmm_likelihood_score_changes(phmm_likelihood *lk, uint32_t n_candidates, const uint64_t *change_off,
                                  const uint32_t *change_node, const uint32_t *change_copy_num,
                                  double *out_logp, double *out_total, uint64_t *out_n_rescored);

/* The current vector becomes current + changes (any change list: one candidate of the last batch, or the union of
 * several, posterior.rs:565-590).  Rescores the reads the move touches (bit-equal to phmm_full_prob_reads_copy_nums on
 * the new vector), shifts the others by ln(T_old / T_new) without accumulating rounding over a chain of moves, updates T.
 * out_total = sum of ln P under the new vector; out_n_rescored = reads run through the kernels; NULL, host or
 * device.  n_changes = 0 changes nothing. */
int phmm_likelihood_move(phmm_likelihood *lk, uint64_t n_changes, const uint32_t *change_node,
                         const uint32_t *change_copy_num, double *out_total, uint64_t *out_n_rescored);

/* What the handle holds: copy_nums[N] (host), per-read ln P [R], their sum (host or device).  Any may be NULL. */
int phmm_likelihood_current(const phmm_likelihood *lk, uint32_t *out_copy_nums, double *out_logp, double *out_total);

/* Rescores the current vector in full (after phmm_model_set_params, or to drop the one rounding of shifted reads).
 * Does not touch the groups. */
int phmm_likelihood_refresh(phmm_likelihood *lk);

/* ---- the handle in the sampler's own units: node groups ---------------------------
 * The sampler's state is a copy-number vector over COMPACT edges (get_copy_nums, CopyNums; UpdateInfo::cycle(),
 * neighbors.rs:193-216), and set_copy_nums writes one compact edge's number into every k-mer of its unitig
 * (multi_dbg.rs:1041-1052).  A group is the node set of one compact edge; the group forms below take and return
 * compact-edge numbers, so that the work in front of the scoring kernels scales with the number of GROUP changes,
 * not with k.
 * Equality with the node form: a group change (g, cn) means (v, cn) for every node v of g.  For any handle state and
 * any group change lists, score_group_changes / move_groups write exactly what score_changes / move write for the
 * expanded lists -- out_logp, out_total, out_n_rescored with the same bits, the same reads rescored -- and after a
 * move the handle is in the same state (phmm_likelihood_current returns the same vector, per-read values and total).
 * Uniform groups: set_groups requires the current vector to be constant within every group.  A later node-form
 * phmm_likelihood_move may change part of a group: that group is then MIXED -- a group-form call that names it is
 * refused, phmm_likelihood_current_groups reports PHMM_GROUP_MIXED for it, every other group keeps working, and
 * phmm_likelihood_set_groups re-validates.  (A node-form move that gives every node of a group one value leaves it
 * uniform at that value.)
 * Refusals are PHMM_EINVAL, write no output and leave vector, T, per-read values and groups as they were: NULL handle
 * or arrays, group_off not starting at 0 or decreasing, a node id >= N, a node in two groups (or twice in one), a
 * group id >= G, a group named twice within one candidate or move, a group-form call with no groups set, a mixed
 * group named.  Empty groups are allowed and are never effective.  Groups belong to the handle and die with it. */
#define PHMM_GROUP_MIXED 0xffffffffu

/* Groups = disjoint sets of PHMM nodes that the sampler changes together: the k-mers of one compact edge
 * (MultiDbg::edges_in_full).  group_off[G+1], group_nodes[group_off[G]], host pointers.  A node may be in no group
 * (it can then only be changed through the node form).  Replaces any earlier groups; n_groups = 0 removes them. */
int phmm_likelihood_set_groups(phmm_likelihood *lk, uint32_t n_groups, const uint64_t *group_off,
                               const uint32_t *group_nodes);
/* phmm_likelihood_score_changes with change_group[] (group ids) in place of change_node[]; outputs NULL, host or
 * device as there; n_candidates = 0 writes nothing. */
int phmm_likelihood_score_group_changes(phmm_likelihood *lk, uint32_t n_candidates, const uint64_t *change_off,
                                        const uint32_t *change_group, const uint32_t *change_copy_num,
                                        double *out_logp, double *out_total, uint64_t *out_n_rescored);
/* phmm_likelihood_move with group ids; n_changes = 0 changes nothing. */
int phmm_likelihood_move_groups(phmm_likelihood *lk, uint64_t n_changes, const uint32_t *change_group,
                                const uint32_t *change_copy_num, double *out_total, uint64_t *out_n_rescored);
/* the current vector in group units: out_group_copy_nums[G] (host), PHMM_GROUP_MIXED for a mixed group */
int phmm_likelihood_current_groups(const phmm_likelihood *lk, uint32_t *out_group_copy_nums);
void phmm_likelihood_destroy(phmm_likelihood *lk);

/* PHMMModel::to_full_prob_sparse_backward (freq.rs:153-163): ln P(read) from PHMMModel::backward_sparse
 * (backward.rs:146-185) -- dense b_step over the last n_warmup positions, then the backward recursion on
 * its own frontier: top_nodes(n_active_nodes) of the previous column, adaptive b_step (backward.rs:216-261).
 *   out_logp[R] = B.tables[0].mb per read;  out_total = their sum.  Either may be NULL or a device pointer.
 * n_warmup = 0 is PHMM_EINVAL (the reference panics in last_table(), table.rs:388). */
int phmm_full_prob_sparse_backward(phmm_model *m, const phmm_reads *reads, double *out_logp,
                                   double *out_total);

/* PHMMModel::run_sparse over a read set (freq.rs:51-55): forward_sparse(use_max_ratio = false) paired with
 * backward_sparse, followed by PHMMOutput::{to_full_prob_forward, to_full_prob_backward, to_node_freqs}
 * (table.rs:482-494; freq.rs:245-255): the product of a dense and a sparse table keeps the sparse operand's
 * elements, of two sparse tables the forward one's (table.rs:320-331).
 *   out_logp_forward[R], out_logp_backward[R], out_node_freq[N] (summed over the reads); any may be NULL or a
 * device pointer.  Keeps the dense head / tail columns and every sparse column of a chunk in HBM. */
int phmm_run_sparse(phmm_model *m, const phmm_reads *reads, double *out_logp_forward,
                    double *out_logp_backward, double *out_node_freq);

/* The backward_sparse tables of ONE read for parity tests / `inspect`-style tools (bin/table.rs:41):
 * b_m/b_i/b_d: [L][N] natural-log values of B.tables[i], -inf where the reference's SparseVec holds no
 * element; b_scal: [L][3] = mb, ib, e; is_dense: [L] 1 for the dense tail.  Any pointer may be NULL.
 * Host pointers. */
int phmm_backward_sparse_tables(phmm_model *m, const uint8_t *read, uint64_t len, double *b_m,
                                double *b_i, double *b_d, double *b_scal, uint8_t *is_dense);

/* Mapping carry-over between graphs: Mapping::map_nodes (hint.rs:60-88) for every read, the carrier of
 * MultiDbg::hint_kp1_from_hint_k (multi_dbg.rs:1325-1335: node of the k-HMM -> the k+1-HMM nodes of its
 * parent edges) and PurgeEdgeMap::update_mapping (multi_dbg.rs:1783-1793: node -> its id after purging, or
 * nothing).  The node map is a CSR over the nodes of the graph the mappings were made on:
 * images of node v = map_nodes[map_off[v] .. map_off[v+1]) (ids of `model_after`'s nodes; may be empty).
 * Per position: prob(image) += prob(node) / |images(node)|, then the 400 most probable, descending.
 * read_logp and read_logp_backward of the result are copied from `mappings`. */
int phmm_mappings_map_nodes(phmm_model *model_after, const phmm_reads *reads,
                            const phmm_mappings *mappings, const uint32_t *map_off,
                            const uint32_t *map_nodes, uint32_t n_nodes_before,
                            phmm_mappings **out);

/* PHMMModel::generate_mappings (hint.rs:193-220): run_with_mapping when `mappings`
 * is given else run_sparse_adaptive(use_max_ratio); then to_mapping_by_score_ratio /
 * to_mapping.  out_node_freq[N] (may be NULL) = Mappings::to_node_freqs.
 * With `mappings` the model must give every read a positive probability on its lists (the reference maps on
 * to_non_zero_phmm, multi_dbg/posterior.rs:609-618): a model that cuts a read -- a k-mer at copy number 0 on its
 * path -- is refused with PHMM_EINVAL; only phmm_full_prob_reads* score such reads (wide-range pass). */
int phmm_generate_mappings(phmm_model *m, const phmm_reads *reads,
                           const phmm_mappings *mappings, int use_max_ratio,
                           phmm_mappings **out, double *out_node_freq);

/* PHMMModel::run_with_mapping (freq.rs:72-76) of every read on its lists, then
 * PHMMOutput::to_edge_and_init_freqs (freq.rs:276-298, 332-389), summed over the reads.
 *   out_logp_forward[R]  per-read ln P of forward_with_mapping;
 *   out_edge_freq[E], out_init_freq[N] as phmm_run_dense_edges defines them.
 * Any output may be NULL or a device pointer.  The cost is that of phmm_generate_mappings with mappings: a list pass,
 * no dense table.  Mappings of another read set are PHMM_EINVAL; so is a model under which a read has probability 0
 * on its lists (as in phmm_generate_mappings with mappings).  Lists of at most 400 nodes, node degree at most 8.
 * Repeated calls on the same inputs return the same bits. */
int phmm_run_with_mapping_edges(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mappings,
                                double *out_logp_forward, double *out_edge_freq, double *out_init_freq);

/* The posterior by state over the lists (to_emit_probs per entry, the head of to_states() per base):
 * phmm_amd_states.h, which includes this header.  This header's symbol table is closed: the ABI tests pin
 * it, and entry points added since are declared in companion headers of their own. */

/* ---- instrumentation ------------------------------------------------------------
 * Device time (ms, HIP events on the call's stream) and launch count of the dominant
 * kernel class in the most recent call of this thread, plus the algorithmic cell
 * count it processed (bench.py's roofline block).  which: 0 = dense forward step,
 * 1 = dense backward+posterior step, 2 = hinted/sparse forward, 3 = sparse backward,
 * 4 = the wide class of the hinted forward (reads whose longest mapping list holds
 * 65-400 nodes, one block per read and candidate group; its launches and time are part
 * of class 2 as well; cells = list entries x candidates it scored; all 0 when the call
 * had no such read or the class is off: it is opt-in, PHMM_WIDE_HINTED=1, and
 * PHMM_NO_WIDE_HINTED=1 wins over that).  Index 4 also covers the list pass: the wide
 * classes on mapping lists.  In phmm_generate_mappings with mappings and in
 * phmm_run_with_mapping_edges it counts the record-storing forward on a block (cells =
 * list entries of its reads) and, for phmm_generate_mappings with use_max_ratio, the
 * list backward on a block (one launch; cells = list entries of the positions it
 * computed).  The developer knob PHMM_NO_WIDE_LIST_BWD=1 keeps that backward on the
 * generic kernel while the forward stays on the block.  With PHMM_WIDE_EDGE_BWD=1 beside
 * PHMM_WIDE_HINTED=1, phmm_run_with_mapping_edges runs its backward half on a block as
 * well and adds that half's launches and cells (list entries of the positions it
 * computed) to index 4; without that knob the call counts its forward half alone.
 * phmm_run_with_mapping_states counts in the same way, its backward half with
 * PHMM_WIDE_STATES_BWD=1 beside PHMM_WIDE_HINTED=1.
 * PHMM_WIDE_BWD_T=128 sends the reads of a block backward whose longest list holds at most
 * 128 nodes to a block of 128 threads (one more launch, the same cells, the same bits);
 * PHMM_WIDE_BWD_T=448 keeps every such read on the block of 448.  Unset, the library takes
 * the small block when a call has more such reads than twice the device's compute units.
 * Any other index is PHMM_EINVAL. */
int phmm_last_call_stats(int which, double *out_ms, uint64_t *out_launches,
                         uint64_t *out_cells);
int phmm_enable_timing(int on);

#ifdef __cplusplus
}
#endif
#endif /* PHMM_AMD_H */
