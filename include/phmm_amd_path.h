/*
 * phmm_amd_path.h -- companion of phmm_amd.h: the best path of every read over its mapping lists (Viterbi).
 *
 * phmm_amd.h's symbol table is closed (the ABI tests pin its entry points one by one); an entry point added
 * after that is declared in a companion header of its own, which includes phmm_amd.h.  The library exports
 * all sets; dbgphmm_amd/_ffi.py lists this header's symbols in EXTENSION_SYMBOLS.
 */
#ifndef PHMM_AMD_PATH_H
#define PHMM_AMD_PATH_H

#include "phmm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PHMM_PATH_NONE      0xffffffffu /* padding of a row; every entry of every row of a read without a path */
#define PHMM_PATH_INS_BEGIN 0xfffffffdu /* the emitting state of the base is InsBegin (no node) */

/* forward_with_mapping (forward.rs:51-75, f_step 276-306) with every sum replaced by a maximum, over the same lists and
 * with the same bound on Del chains, in natural logs.  Read x[0..L-1], S_p the list of position p, G = n_max_gaps,
 * e_v(x) = p_match_emit, t_uv = trans_logp, init_v = init_logp.  A value read at a node that is not on the list it is
 * read from is -inf; a node listed twice is looked up at its first entry.  Column -1: MB = 0, IB = -inf, no node values.
 *   M_p[v]  = e_v(x_p) + max( max over edges u->v, u in S_{p-1}, of
 *                               t_uv + max(p_MM + M_{p-1}[u], p_IM + I_{p-1}[u], p_DM + D_{p-1}[u]),
 *                             init_v + max(p_MM + MB_{p-1}, p_IM + IB_{p-1}) )
 *   I_p[v]  = p_random + max(p_MI + M_{p-1}[v], p_II + I_{p-1}[v], p_DI + D_{p-1}[v])
 *   MB_p    = -inf,   IB_p = p_random + max(p_MI + MB_{p-1}, p_II + IB_{p-1})
 *   D0_p[v] = max( max over u->v, u in S_p, of t_uv + max(p_MD + M_p[u], p_ID + I_p[u]),
 *                  init_v + max(p_MD + MB_p, p_ID + IB_p) )
 *   Dt_p[v] = max over u->v, u in S_p, of t_uv + p_DD + D(t-1)_p[u]      t = 1..G
 *   D_p[v]  = max over t = 0..G of Dt_p[v]
 *   best    = p_end + max over v in S_{L-1} of max(M, I, D)_{L-1}[v]
 * A path is, per base, one emitting state (Match or Ins of a listed node, or InsBegin) and then 0 to G + 1 Del states on
 * nodes of the same list; Dels behind the last base count.  Every such path is a term of the sum forward_with_mapping
 * computes, so best <= its ln P on the same lists.  Parameters of -inf are legal; nothing is NaN.
 *
 *   out_logp[R]                  best per read; -inf for a read with no path of positive probability on its lists and
 *                                for an empty read (a result, not a refusal);
 *   out_path[total_bases][stride]  stride = n_max_gaps + 2 of the model's parameters at the call (at most 8).  Row
 *                                g = read_off[r] + p: entry 0 is the emitting state of base p, (slot << 2) | 0 for
 *                                Match, (slot << 2) | 1 for Ins, slot the index into list p of the input CSR (the node
 *                                is nodes[pos_off[g] + slot]), or PHMM_PATH_INS_BEGIN; entries 1.. are the Del states
 *                                passed behind it, in order, as (slot << 2) | 2; the rest is PHMM_PATH_NONE.  Every
 *                                row of a read whose value is -inf is all PHMM_PATH_NONE;
 *   out_counts[R][4]             read off the path: Match states whose node emits the read's base, Match states whose
 *                                node does not, Ins states (InsBegin included), Del states.  Zeros without a path.
 *
 * TIES.  Every maximum above is taken over candidates in a fixed order of rank: a candidate replaces the one held when
 * its value (the whole term, e.g. t_uv + (p_IM + I_{p-1}[u])) is greater, or exactly equal and its rank lower; -inf is
 * never chosen.  The rank of a source of Match and of an end state is (slot << 2) | kind, kind 0 Match, 1 Ins, 2 Del:
 * the earlier list entry first, within an entry Match before Ins before Del; Begin / InsBegin comes behind every node
 * state.  The sources of Ins rank Match, Ins, Del; those of Del level 0 by (slot << 1) | (0 Match, 1 Ins), InsBegin last;
 * the parents of a Del level by slot; among the Del levels of an entry the lower level.  Parallel edges u->v contribute
 * one candidate each with the same rank, so the heavier edge decides.  The forward pass records what it chose and the
 * walk back follows the record; the end state is chosen by the same rule.
 *
 * Any output may be NULL, a host pointer or a device pointer; with out_path == NULL no path leaves the device.
 * Refusals are those of phmm_run_with_mapping_states, with nothing written: NULL model, reads or mappings and mappings
 * of another read set PHMM_EINVAL, a list of more than 400 nodes PHMM_ECAPACITY, node degree above 8 PHMM_EINVAL.  A
 * list that names a node >= the model's node count is PHMM_EINVAL too: the host checks the lists before any launch.  No
 * reads: nothing is written.  Repeated calls return the same bits, and a read's three outputs do not depend on which
 * other reads are in the call.  The back-pointers (16 bytes per list entry) come from the device workspace; under
 * phmm_set_workspace_limit the reads run in chunks.  Index 2 of phmm_last_call_stats counts the call's device time,
 * launches and cells (list entries), as for the hinted forward. */
int phmm_run_with_mapping_best_path(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mappings,
                                    double *out_logp, uint32_t *out_path, uint32_t *out_counts);

#ifdef __cplusplus
}
#endif
#endif /* PHMM_AMD_PATH_H */
