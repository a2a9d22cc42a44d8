/*
 * phmm_amd_generate.h -- companion of phmm_amd.h: reads drawn from the model itself, the generative direction
 * (sample_rng_from, sample.rs:270-321, with make_transition, make_emission and the pickers of sample/picker.rs).
 *
 * phmm_amd.h's symbol table is closed (the ABI tests pin its entry points one by one); an entry point added
 * after that is declared in a companion header of its own, which includes phmm_amd.h.  The library exports
 * all sets; dbgphmm_amd/_ffi.py lists this header's symbols in EXTENSION_SYMBOLS.
 */
#ifndef PHMM_AMD_GENERATE_H
#define PHMM_AMD_GENERATE_H

#include "phmm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PHMM_GEN_STATE_COUNT 0u  /* ReadLength::StateCount(length): p_end is not a candidate          */
#define PHMM_GEN_ENDABLE     1u  /* ReadLength::Endable(length): End is a candidate with term p_end   */
#define PHMM_GEN_EMIT_COUNT  2u  /* ReadLength::EmitCount(length): stop after `length` bases, no End  */
#define PHMM_GEN_END         0xfffffffcu  /* history word of the End state                            */
/* out_flags bits */
#define PHMM_GEN_ENDED 1u             /* End was drawn                                                 */
#define PHMM_GEN_DEAD_END 2u          /* no child / no init node of positive probability: End, no draw */
#define PHMM_GEN_STATE_CAP 4u         /* stopped at the hard bound on states (below)                   */
#define PHMM_GEN_HISTORY_TRUNCATED 8u /* more states than history_cap; bases and flags are unaffected  */

/* THE WALK.  Walk w of a call has index i = first_index + w.  It starts in MatchBegin or, when start_nodes is given, in
 * Match(v) with v drawn among start_nodes in the order given, terms init_v (pick_init_node_from).  Such a start emits
 * first (one emission decision); it is the first word of the history and counts in out_node_usage, but it is not a state
 * of the length count.  Then the walk takes steps; t_vw = trans_logp, init_v = init_logp, all terms natural logs.
 * One step from state X (Match, Ins or Del) on node v:
 *   1. the child: candidates the out-edges of v in ascending edge index, terms t_vw; parallel edges are one candidate
 *      each.  (The child is drawn even when Ins is chosen afterwards, as the reference does.)
 *   2. the next state: candidates in this order Match(child), Ins(v), Del(child) and, under PHMM_GEN_ENDABLE, End; terms
 *      p_XM, p_XI, p_XD, p_end.
 *   3. the emission.  Match: candidates A, C, G, T with term p_match for the node's emission and p_mismatch for the
 *      others; on a node whose emission is none of the four all four have p_mismatch.  Ins and InsBegin: A, C, G, T with
 *      term p_random, still one draw.  Del and End emit nothing and consume no draw.
 * One step from MatchBegin or InsBegin:
 *   1. the init node: candidates all nodes in ascending id, terms init_v;
 *   2. the state: from MatchBegin the candidates in order InsBegin, Match(v), Del(v) with terms p_MI, p_MM, p_MD; from
 *      InsBegin the terms are p_II, p_IM, p_ID;
 *   3. the emission, as above.
 * A decision none of whose candidates has positive weight -- a node without a child of finite t_vw, no init node of
 * finite init_v, and likewise a state or emission decision whose terms are all -inf (the reference panics there) -- ends
 * the walk: the state entered is End, the flag PHMM_GEN_DEAD_END, and no draw is consumed.
 * After every step the walk stops when the state is End (drawn: PHMM_GEN_ENDED); else when the count its length_kind
 * names has reached `length` -- states entered by steps for kinds 0 and 1, bases for kind 2 --; else when it has taken
 * 8 * length + 64 steps (PHMM_GEN_STATE_CAP).  The bound exists because every other exit depends on the parameters:
 * p_DD = 1 on a cycle would otherwise never return.  Such a walk is a result with a flag.  A walk emits at most
 * length + 1 bases.
 *
 * THE RANDOM STREAM.  mix(z) is the SplitMix64 finaliser: z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27;
 * z *= 0x94D049BB133111EB; z ^= z >> 31 (64-bit unsigned arithmetic).  GOLD = 0x9E3779B97F4A7C15.  Walk i -- its index
 * first_index + w, not its place in the call or in a chunk -- starts at x0 = mix(seed ^ mix(i + GOLD)); draw d = 1, 2, ..
 * of that walk is u = (mix(x0 + d * GOLD) >> 11) * 2^-53, in [0, 1).
 *
 * THE DRAW RULE.  A decision has candidates in a fixed order with log terms t_i.  w_i = exp(t_i - max t), 0 for -inf;
 * c_i is the running sum of the w in that order (sequential double additions); the choice is the smallest i with
 * u * c_last < c_i, and if none qualifies (rounding at the top) the last candidate with w > 0.  Every decision consumes
 * exactly one draw, a decision with a single candidate included.
 *
 *   out_bases[n_walks][length + 1]     ASCII bases, padded with 0; the stride is length + 1 in every mode;
 *   out_len[n_walks]                   bases of the walk;
 *   out_flags[n_walks]                 PHMM_GEN_* flag bits;
 *   out_history[n_walks][history_cap]  one word per state entered, in order, a start node's Match first: (node << 2) |
 *                                      kind with the kinds of phmm_amd_path.h (0 Match, 1 Ins, 2 Del),
 *                                      PHMM_PATH_INS_BEGIN, or PHMM_GEN_END; padding PHMM_PATH_NONE;
 *   out_history_len[n_walks]           the untruncated number of history words;
 *   out_node_usage[n_nodes]            Match + Ins + Del states of all walks of the call per node: a recount of the
 *                                      untruncated histories.  The call clears it, then adds with 32-bit integer atomics.
 * Each output may be NULL, a host pointer or a device pointer; start_nodes is a host pointer.
 * PHMM_GEN_HISTORY_TRUNCATED is set when history_cap > 0 and the walk has more history words; it depends on history_cap
 * alone, not on whether out_history is given.
 *
 * Refusals, all PHMM_EINVAL with nothing written: NULL model; length == 0; length >= 2^28; a length_kind that is not one
 * of the three; start_nodes == NULL while n_start_nodes is positive (or n_start_nodes >= 2^32); a start node >= n_nodes;
 * start nodes none of which has init > -inf (the reference panics here); out_history given with history_cap == 0;
 * out_history given with n_nodes > 2^30.  n_walks == 0 writes nothing and returns PHMM_OK.
 *
 * Walk i depends only on the model, seed, i, length, length_kind and the start nodes (the truncation flag: history_cap):
 * not on first_index, n_walks, the other walks, where the outputs live, which outputs were requested, or the chunks the
 * walks run in under phmm_set_workspace_limit.  Repeated calls give the same bits.  The running sums of the init pick and
 * of every node's child pick are built once per model on the host, in candidate order, and kept until
 * phmm_model_set_probs; the device finds the init node by binary search, which equals the linear scan because c is
 * non-decreasing.  Staging rows come from the device workspace.
 * Index 2 of phmm_last_call_stats counts the call's device time, launches and cells (steps taken). */
int phmm_sample_reads(phmm_model *m, uint64_t first_index, uint64_t n_walks, uint32_t length, uint32_t length_kind,
                      const uint32_t *start_nodes, uint64_t n_start_nodes, uint64_t seed,
                      uint8_t *out_bases, uint32_t *out_len, uint32_t *out_flags,
                      uint32_t *out_history, uint32_t history_cap, uint32_t *out_history_len,
                      uint32_t *out_node_usage);

#ifdef __cplusplus
}
#endif
#endif /* PHMM_AMD_GENERATE_H */
