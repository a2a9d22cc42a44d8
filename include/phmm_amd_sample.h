/*
 * phmm_amd_sample.h -- companion of phmm_amd.h: draws from the posterior over paths of every read over its mapping
 * lists, P(path | read, model, lists).  The forward sums are the filter; every sample is one random walk back.
 *
 * phmm_amd.h's symbol table is closed (the ABI tests pin its entry points one by one); an entry point added
 * after that is declared in a companion header of its own, which includes phmm_amd.h.  The library exports
 * all sets; dbgphmm_amd/_ffi.py lists this header's symbols in EXTENSION_SYMBOLS.
 */
#ifndef PHMM_AMD_SAMPLE_H
#define PHMM_AMD_SAMPLE_H

#include "phmm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PHMM_SAMPLE_MAX 64 /* samples per call; for more, call again with another seed */

/* THE MODEL is the one phmm_amd_path.h writes out with every max replaced by a sum, in natural logs: the same lists, the
 * same bound on Del chains (levels 0..G, G = n_max_gaps), column -1 with MB = 0 and IB = -inf, -inf parameters legal.
 *   lse(t_1, .., t_n) = mx + ln( (..(w_1 + w_2) + ..) + w_n ),  mx = max t_i,  w_i = exp(t_i - mx), 0 for t_i = -inf;
 *                       -inf when no t_i is finite.  The terms are added in the order written.
 *   M_p[v]  = e_v(x_p) + lse( for every edge u->v in ascending edge index with u in S_{p-1}:
 *                               t_uv + (p_MM + M_{p-1}[u]), t_uv + (p_IM + I_{p-1}[u]), t_uv + (p_DM + D_{p-1}[u]);
 *                             last init_v + p_MM at p = 0, init_v + (p_IM + IB_{p-1}) otherwise )
 *   I_p[v]  = p_random + lse(p_MI + M_{p-1}[v], p_II + I_{p-1}[v], p_DI + D_{p-1}[v])       (-inf if v is not in S_{p-1})
 *   IB_p    = p_random + p_MI at p = 0, p_random + (p_II + IB_{p-1}) otherwise
 *   D0_p[v] = lse( for every edge u->v in ascending edge index with u in S_p:
 *                    t_uv + (p_MD + M_p[u]), t_uv + (p_ID + I_p[u]);  last init_v + (p_ID + IB_p) )
 *   Dt_p[v] = lse( the same edges: t_uv + (p_DD + D(t-1)_p[u]) )                              t = 1..G
 *   D_p[v]  = lse(D0_p[v], .., DG_p[v])
 *   ln Z    = p_end + lse( for every entry of S_{L-1} in slot order: M, I, D )
 * DUPLICATES.  A node listed twice in one list holds states at its FIRST entry only; every value of a later entry is -inf
 * and it is never on a sampled path.  A value read at a node is read at its first entry.  So ln Z is the forward total
 * over the lists as sets, the quantity phmm_full_prob_reads returns for the same lists.
 *
 * THE RANDOM STREAM.  mix(z) is the SplitMix64 finaliser: z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27;
 * z *= 0x94D049BB133111EB; z ^= z >> 31 (64-bit unsigned arithmetic).  GOLD = 0x9E3779B97F4A7C15.  Read r -- its index
 * in the read set, not in a chunk -- and sample s start at x0 = mix(seed ^ mix(r * 64 + s + GOLD)); draw d = 1, 2, .. of
 * that walk is u = (mix(x0 + d * GOLD) >> 11) * 2^-53, in [0, 1).
 *
 * THE DRAW RULE.  A decision has candidates in a fixed order with log terms t_i.  w_i = exp(t_i - max t), 0 for -inf;
 * c_i is the running sum of the w in that order; the choice is the smallest i with u * c_last < c_i, and if none
 * qualifies (rounding at the top) the last candidate with w > 0.  Every decision consumes exactly one draw, a decision
 * with a single candidate included.  The walk starts at the end and goes back:
 *   1. the end state: every entry of the last list in slot order, within an entry M, I, D; terms M, I, D (the lse of its
 *      levels);
 *   2. in a Del of entry j: first the level, candidates 0..G with terms Dt[j].  Then per level t >= 1, going down, the
 *      parent: the incoming edges u->v of the node with u in the same list, in ascending edge index, u's first entry q the
 *      slot, terms t_uv + (p_DD + D(t-1)[q]).  Then the source of level 0: the same edges in the same order, within an
 *      edge M then I, terms t_uv + (p_MD + M[q]) and t_uv + (p_ID + I[q]); last InsBegin, init_v + (p_ID + IB_p);
 *   3. in a Match of entry j at position p: the incoming edges with u in list p - 1, in ascending edge index, within an
 *      edge M, I, D, terms t_uv + (p_XM + X_{p-1}[q]); last Begin, init_v + p_MM at p = 0 and init_v + (p_IM + IB_{p-1})
 *      otherwise.  Begin at p = 0 ends the walk; otherwise the walk stands in InsBegin at p - 1;
 *   4. in an Ins of entry j: M, I, D of the same node's first entry in list p - 1, terms p_XI + X_{p-1}[q];
 *   5. InsBegin has one predecessor and consumes no draw.
 * Parallel edges u->v are one candidate each.
 *
 *   out_logp[R]                     ln Z per read; -inf for an empty read and for a read with no path (a result, not a
 *                                   refusal);
 *   out_path_logp[R][S]             ln P of each sampled path: p_end plus the path's own terms (emission, transition and
 *                                   edge or init per state), added up during the walk; -inf without a path;
 *   out_path[S][total_bases][stride]  plane s is sample s of every read, rows exactly as phmm_amd_path.h encodes them
 *                                   (stride = n_max_gaps + 2, (slot << 2) | kind, PHMM_PATH_INS_BEGIN, PHMM_PATH_NONE);
 *                                   all PHMM_PATH_NONE for a read without a path;
 *   out_counts[R][S][4]             matches, mismatches, Ins (InsBegin included) and Dels of each sample; zeros without
 *                                   a path;
 *   out_node_usage[S][n_nodes]      per sample the number of Match, Ins and Del states of all reads on each node: one
 *                                   draw of what the node frequencies are the expectation of.  The call clears it and
 *                                   adds into it with 32-bit integer atomics, so the result does not depend on order.
 *
 * Any output may be NULL, a host pointer or a device pointer.  Refusals are those of phmm_run_with_mapping_best_path,
 * with nothing written; n_samples == 0 and n_samples > PHMM_SAMPLE_MAX are PHMM_EINVAL besides.  No reads: nothing is
 * written.  A read's outputs depend on the model, the read, its lists, seed, its index r and s alone: not on the other
 * reads of the call, on the capacity class its lists fall in, on chunking under phmm_set_workspace_limit, or on where the
 * outputs live; repeated calls return the same bits, and sample s of a call with fewer samples is sample s of a call with
 * more.  The forward records (128 bytes per list entry) come from the device workspace; under a workspace limit the reads
 * run in chunks.  Index 2 of phmm_last_call_stats counts the call's device time, launches and cells (list entries). */
int phmm_run_with_mapping_sample_paths(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mappings,
                                       uint32_t n_samples, uint64_t seed,
                                       double *out_logp, double *out_path_logp, uint32_t *out_path,
                                       uint32_t *out_counts, uint32_t *out_node_usage);

#ifdef __cplusplus
}
#endif
#endif /* PHMM_AMD_SAMPLE_H */
