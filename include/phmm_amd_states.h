/*
 * phmm_amd_states.h -- companion of phmm_amd.h: the posterior by state over mapping lists.
 *
 * phmm_amd.h's symbol table is closed (the ABI tests pin its entry points one by one); an entry point added
 * after that is declared in a companion header of its own, which includes phmm_amd.h.  The library exports
 * both sets; dbgphmm_amd/_ffi.py lists this header's symbols in EXTENSION_SYMBOLS.
 */
#ifndef PHMM_AMD_STATES_H
#define PHMM_AMD_STATES_H

#include "phmm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* PHMMModel::run_with_mapping (freq.rs:72-76) of every read on its lists, then per read position
 * PHMMOutput::to_emit_probs(p + 1) (table.rs:500-505) by state, and the head of its to_states() (table.rs:215-254).
 * Read r of length L, position p in 0..L-1, global position g = read_off[r] + p; entry a runs over
 * [pos_off[g], pos_off[g+1]) of the INPUT mappings, v = nodes[a], slot = a - pos_off[g].
 *   out_logp_forward[R]            per-read ln P of forward_with_mapping (as in phmm_run_with_mapping_edges);
 *   out_state_logp[total_entries][3]  [3a + s], s = 0, 1, 2 (Match, Ins, Del) =
 *                                  ln(F.tables[p].s[v] * B.table_merged(p+1).s[v] / P), natural logs, -inf for a zero
 *                                  probability.  B.table_merged(L) is b_init (p_end in every state of every node);
 *                                  B.tables[p+1] lives on the list of position p+1: a node of list p that list p+1
 *                                  does not hold has B = 0, i.e. -inf in its three states;
 *   out_best[total_bases]          (slot << 2) | kind, kind 0 = Match, 1 = Ins, 2 = Del, of the largest of the
 *                                  position's 3n values as written to out_state_logp; among exactly equal values Del
 *                                  before Ins before Match, and within a kind the later slot (the reference sorts
 *                                  ascending, stable, and reverses).  0xffffffff where the list is empty or every
 *                                  value is -inf.  Computed the same with out_state_logp == NULL: 4 bytes per base
 *                                  leave the device instead of 24 per entry.
 * Any output may be NULL or a device pointer.  Refusals are those of phmm_run_with_mapping_edges, with nothing
 * written: NULL model, reads or mappings and mappings of another read set PHMM_EINVAL, a list of more than 400 nodes
 * PHMM_ECAPACITY, node degree above 8, a model under which a read has probability 0 on its lists PHMM_EINVAL.
 * No reads: nothing is written.  Repeated calls on the same inputs return the same bits.
 * With PHMM_WIDE_STATES_BWD=1 beside PHMM_WIDE_HINTED=1 the backward half of reads whose longest list holds 65-400
 * nodes runs on a block, as PHMM_WIDE_EDGE_BWD does for phmm_run_with_mapping_edges; PHMM_NO_WIDE_HINTED=1 and
 * PHMM_NO_WIDE_LIST_BWD=1 win over it, PHMM_WIDE_BWD_T chooses the block size, and index 4 of phmm_last_call_stats
 * counts both halves as it does for that call. */
int phmm_run_with_mapping_states(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mappings,
                                 double *out_logp_forward, double *out_state_logp, uint32_t *out_best);

#ifdef __cplusplus
}
#endif
#endif /* PHMM_AMD_STATES_H */
