/*
 * phmm_amd_mea.h -- companion of phmm_amd.h: the maximum-expected-accuracy (MEA) path of every read over its mapping
 * lists, and the weighted walk it is built on.
 *
 * phmm_amd.h's symbol table is closed (the ABI tests pin its entry points one by one); an entry point added
 * after that is declared in a companion header of its own, which includes phmm_amd.h.  The library exports
 * all sets; dbgphmm_amd/_ffi_mea.py lists this header's symbols in MEA_SYMBOLS and binds them.
 */
#ifndef PHMM_AMD_MEA_H
#define PHMM_AMD_MEA_H

#include "phmm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* THE WEIGHTED WALK.  phmm_run_with_mapping_best_path (phmm_amd_path.h) returns the legal walk of the largest
 * probability; this call returns the legal walk of the largest summed WEIGHT, the weights being the caller's, one per
 * list entry and kind.  The model's log probabilities decide only which walks are legal.
 *
 * The path family is exactly that of phmm_amd_path.h: per base one emitting state (Match or Ins of a listed node, or
 * InsBegin), then 0 to G + 1 Del states on nodes of the same list, G = n_max_gaps; Dels behind the last base count; a
 * value read at a node that is not on the list it is read from is -inf; a node listed twice is looked up at its first
 * entry.  (Every entry has its own weights here, so the last clause shows: a state on a later entry of its node is
 * computed and may end the path, but nothing continues from it.)
 *
 *   weights[total_entries][3]   [3a + s], s = 0, 1, 2: the weight of Match, Ins, Del of entry a of the mappings' CSR
 *                               (the layout of out_state_logp of phmm_run_with_mapping_states); every one a finite double;
 *   ib_weight[total_bases]      the weight of InsBegin emitting base g; NULL: 0 everywhere.
 *
 * ADMISSIBLE.  A transition is admissible when the term the recursion of phmm_amd_path.h would add for it is greater
 * than -inf: t_uv + p_MM, t_uv + p_IM, t_uv + p_DM into a Match over the edge u->v; init_v + p_MM (base 0) or
 * init_v + p_IM (behind InsBegin) into a Match from Begin / InsBegin; p_MI, p_II, p_DI into an Ins (and p_MI, p_II
 * along the InsBegin chain); t_uv + p_MD, t_uv + p_ID into Del level 0, init_v + p_ID from InsBegin; t_uv + p_DD from
 * one Del level to the next.  Parallel edges u->v give one candidate each.  A Match of node v at base p is admissible
 * only if e_v(x_p) > -inf (p_match or p_mismatch, whichever applies); Ins and InsBegin only if p_random > -inf; the end
 * only if p_end > -inf.
 *
 * VALUES.  Begin has value 0.  The value of a state is its own weight plus the maximum, over its admissible sources
 * whose value is greater than -inf, of the source's value; a state that no admissible path reaches has value -inf, and
 * with finite weights that is the only way -inf arises.  With S_p the list of position p, w_M / w_I / w_D the weights of
 * the entry of v in S_p and [c] a = a if the condition c holds, -inf otherwise:
 *   M_p[v]  = [e_v(x_p) > -inf] max( max over edges u->v, u in S_{p-1}, of
 *                                      max([t_uv + p_MM > -inf] M_{p-1}[u], [t_uv + p_IM > -inf] I_{p-1}[u],
 *                                          [t_uv + p_DM > -inf] D_{p-1}[u]),
 *                                    p = 0: [init_v + p_MM > -inf] 0,  p > 0: [init_v + p_IM > -inf] IB_{p-1} )  + w_M
 *   I_p[v]  = [p_random > -inf] max([p_MI > -inf] M_{p-1}[v], [p_II > -inf] I_{p-1}[v], [p_DI > -inf] D_{p-1}[v])  + w_I
 *   IB_p    = [p_random > -inf] (p = 0: [p_MI > -inf] 0,  p > 0: [p_II > -inf] IB_{p-1})  + ib_weight[p]
 *   D0_p[v] = max( max over u->v, u in S_p, of max([t_uv + p_MD > -inf] M_p[u], [t_uv + p_ID > -inf] I_p[u]),
 *                  [init_v + p_ID > -inf] IB_p )  + w_D
 *   Dt_p[v] = max over u->v, u in S_p, of [t_uv + p_DD > -inf] D(t-1)_p[u]  + w_D          t = 1..G
 *   D_p[v]  = max over t = 0..G of Dt_p[v]
 *   score   = [p_end > -inf] max over v in S_{L-1} of max(M, I, D)_{L-1}[v]
 * Every "+ w" is one IEEE double addition fl(source value + own weight), so the value of a path is its weights summed
 * left to right in path order (the emitting state of a base, then each Del in the order passed).  Rounding is
 * monotone, so the maximum the recursion reaches equals the maximum, over all legal paths, of that left-to-right sum.
 *
 * TIES go by the rule of phmm_amd_path.h, word for word: every maximum is taken over candidates in a fixed order of
 * rank; a candidate replaces the one held when its value (here: the source's value) is greater, or exactly equal and
 * its rank lower; -inf is never chosen.  The rank of a source of Match and of an end state is (slot << 2) | kind, kind
 * 0 Match, 1 Ins, 2 Del; Begin / InsBegin comes behind every node state.  The sources of Ins rank Match, Ins, Del;
 * those of Del level 0 by (slot << 1) | (0 Match, 1 Ins), InsBegin last; the parents of a Del level by slot; among the
 * Del levels of an entry -- which all carry the entry's one Del weight here -- the lower level.  The forward pass
 * records what it chose and the walk back follows the record.
 *
 *   out_score[R]                   the value of the best end state; -inf for a read without a legal path and for an
 *                                  empty read (a result, not a refusal);
 *   out_path[total_bases][stride]  exactly the rows of phmm_run_with_mapping_best_path, stride = n_max_gaps + 2: entry
 *                                  0 the emitting state, (slot << 2) | 0 Match / 1 Ins or PHMM_PATH_INS_BEGIN, then
 *                                  the Del states behind it as (slot << 2) | 2, then PHMM_PATH_NONE; all
 *                                  PHMM_PATH_NONE (0xffffffff) for a read without a path;
 *   out_counts[R][4]               as there: matches, mismatches, insertions (InsBegin included), deletions.
 *
 * Any output may be NULL, a host pointer or a device pointer; weights and ib_weight may be host or device pointers
 * (host arrays are uploaded once per call).  Refusals, with nothing written: those of the best-path call (NULL model,
 * reads or mappings and mappings of another read set PHMM_EINVAL, a list of more than 400 nodes PHMM_ECAPACITY, node
 * degree above 8 and a listed node >= the node count PHMM_EINVAL); weights == NULL PHMM_EINVAL; any weight, of an entry
 * or of InsBegin, that is NaN or infinite PHMM_EINVAL -- a check pass on the device finds these before the first
 * forward launch, and no index is ever derived from a weight.  No reads: nothing is written.
 * The back-pointers (16 bytes per list entry) come from the device workspace; under phmm_set_workspace_limit the reads
 * run in chunks, and uploaded weights count against the limit.  A read's outputs depend on the read, its lists and its
 * weights alone; repeated calls return the same bits.  Index 2 of phmm_last_call_stats counts the call's device time,
 * launches and cells (list entries), as for the best path. */
int phmm_run_with_mapping_weighted_path(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mappings,
                                        const double *weights, const double *ib_weight,
                                        double *out_score, uint32_t *out_path, uint32_t *out_counts);

/* THE MEA PATH: the legal walk whose states have the largest summed posterior.  The call runs
 * phmm_run_with_mapping_states (phmm_amd_states.h) on the lists with its per-entry values kept on the device, turns
 * them into weights with one kernel,
 *   w_M = exp(state_logp_M),   w_I = exp(state_logp_I),   w_D = del_weight * exp(state_logp_D),   exp(-inf) = 0 exactly,
 * and puts the weights through the weighted walk above.  InsBegin has weight 0: its posterior is not among the outputs
 * of the states call, so a base the path gives to InsBegin adds nothing to the score.
 * del_weight must be finite and >= 0, else PHMM_EINVAL.  At 1 the score is the expected number of the path's states,
 * emitting and Del, that the true path shares at the same base; at 0 it counts emitting states only.
 *
 *   out_logp_forward[R]            that of the states call, bit for bit;
 *   out_score, out_path, out_counts  as for the weighted walk;
 *   out_weights[total_entries][3]  (optional) the weights actually used: phmm_run_with_mapping_weighted_path on them
 *                                  returns the same score, rows and counts bit for bit.
 *
 * Any output may be NULL, a host pointer or a device pointer.  Refusals are those of the states call, with nothing
 * written, a read of probability 0 on its lists included (PHMM_EINVAL).  The weights plane (24 bytes per entry, the
 * whole call) counts against the workspace: if it alone exceeds phmm_set_workspace_limit the call returns
 * PHMM_ECAPACITY with nothing written; the walk behind it runs in chunks as above.  The environment knobs of the states
 * pass (PHMM_WIDE_HINTED, PHMM_WIDE_STATES_BWD and the others) act on its states half as documented there.  Index 2 of
 * phmm_last_call_stats counts the walk alone; the other indices are those of the states half. */
int phmm_run_with_mapping_mea_path(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mappings,
                                   double del_weight, double *out_logp_forward, double *out_score,
                                   uint32_t *out_path, uint32_t *out_counts, double *out_weights);

#ifdef __cplusplus
}
#endif
#endif /* PHMM_AMD_MEA_H */
