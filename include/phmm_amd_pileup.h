/*
 * phmm_amd_pileup.h -- companion of phmm_amd.h: per read and node, the posterior by state split by the base the read
 * showed there, over its mapping lists, and its sum over the reads: a pileup on the graph.
 *
 * phmm_amd.h's symbol table is closed (the ABI tests pin its entry points one by one); an entry point added
 * after that is declared in a companion header of its own.  This one includes phmm_amd_usage.h, whose handle and
 * accessors carry the rows.  The library exports all sets; dbgphmm_amd/_ffi_pileup.py lists this header's symbol in
 * PILEUP_SYMBOLS and binds it.
 */
#ifndef PHMM_AMD_PILEUP_H
#define PHMM_AMD_PILEUP_H

#include "phmm_amd_usage.h"

#ifdef __cplusplus
extern "C" {
#endif

/* PILEUP.  phmm_run_with_mapping_read_usage (phmm_amd_usage.h) says how often a read used a node, by state; this call
 * keeps, beside that, which base the read showed there.  At a Match the read base agrees or disagrees with the node's
 * emission; at an Ins it is an inserted base hanging on that node.
 *
 * The call runs phmm_run_with_mapping_states (phmm_amd_states.h) with its per-entry values kept on the device and
 * reduces them there; state_logp below is what that call writes for the same inputs and knobs.  Entry a of the
 * mappings' CSR lies at read position p of read r; its node is v = nodes[a]; the read base x is the base of r at p, and
 * its base code is c(x): A 0, C 1, G 2, T 3.
 *
 * POSITION of an entry.  With pos_off[] the offsets of the lists of all positions of all reads in a row, the position
 * of entry a is the last g with pos_off[g] <= a < pos_off[g + 1]: empty lists before, between and behind are passed
 * over (an empty list holds no entry).  g lies within the read of the entry; p = g - (the first position of r).
 *
 * KEY.  The key of an entry is 4 * v + c(x); there are K = 4 * N keys (N the node count).
 *
 * ROW of read r: the rows come back as a phmm_read_usage handle (phmm_amd_usage.h) with phmm_read_usage_keys() == 4N.
 * A row holds the distinct keys among the entries of r, in ascending order -- the entries row_off[r] ..
 * row_off[r + 1] - 1 of keys[] and usage[][3].
 *   usage[e][s], s = 0 Match, 1 Ins, 2 Del:  the sum of exp(state_logp[a][s]) over the read's entries a with that key;
 *   exp(-inf) is exactly 0.
 * The order of the sums is the one phmm_amd_usage.h gives (ORDER OF THE SUMS: the n <= 64 and n > 64 rules), over the
 * segment of one read and one key in the order of the CSR.  Which keys a row holds is decided by the lists alone: a key
 * whose terms are all 0 stays, with zeros.  A node listed twice at a position counts twice in the reduction, as in
 * phmm_amd_usage.h; the forward pass of the states half as it stands refuses such a list (PHMM_EINVAL, "duplicate node
 * in a mapping list"), so today that case ends as a refusal.
 * The Del state emits nothing: the Del value under key (v, c) is the Del mass of v at the positions whose base is c,
 * and only its sum over c has a meaning of its own.
 * The existing phmm_read_usage_reads / _keys / _total / _export / _destroy serve unchanged; no handle type is added.
 *
 *   out_logp_forward[R]    that of the states call, bit for bit;
 *   out_node_pileup[N][9]  the totals over all reads.  COLUMNS: 0-3 the Match mass of node v by read base A C G T,
 *                          4-7 the Ins mass by read base, 8 the Del mass.  Column c and column 4 + c of v are the sums
 *                          of the row entries with key 4 v + c, taken in read order by the one-wave rule: 64 lane-strided
 *                          partial sums p_l = ((0 + t_l) + t_{l+64}) + ..., then p_l <- p_l + p_{l xor d}, d = 32, 16, 8,
 *                          4, 2, 1, the result p_0 -- for any n.  Column 8 sums the Del values of the rows with the keys
 *                          4 v .. 4 v + 3 in sorted order (key, then read) by the same rule.  A node in no row gets
 *                          zeros;
 *   *out                   the rows; out == NULL: scores and totals only.
 * Each output pointer may be NULL, a host pointer or a device pointer.
 *
 * BITS.  There are no floating-point atomics.  A read's row depends on the model, the read and its lists alone -- not
 * on the other reads, the chunking under phmm_set_workspace_limit, the capacity class or where the outputs live -- and
 * repeated calls return the same bits.
 *
 * REFUSALS, with nothing written and *out left as it was: those of phmm_run_with_mapping_read_usage (its group
 * refusals apart: this call takes no groups); PHMM_EINVAL for a read holding a byte other than A C G T (lowercase and
 * N included), the message naming the read and the position, checked on the host before any device work;
 * PHMM_ECAPACITY for N > 2^30 - 1, where the key does not fit 32 bits beside the no-key value; PHMM_ECAPACITY when
 * out_node_pileup is asked for over more than 2^31 - 2 row entries.
 * NO READS: no output array is written, and *out is a handle of 0 rows.
 *
 * WORKSPACE and STATISTICS are those of phmm_run_with_mapping_read_usage: the plane of 24 bytes per list entry, chunks
 * of consecutive whole reads under phmm_set_workspace_limit, the sort behind the totals not chunked.  Index 2 of
 * phmm_last_call_stats counts the reduction alone -- device time, launches, cells = list entries.  The call has no knob
 * of its own. */
int phmm_run_with_mapping_pileup(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mappings,
                                 double *out_logp_forward, double *out_node_pileup, phmm_read_usage **out);

#ifdef __cplusplus
}
#endif
#endif /* PHMM_AMD_PILEUP_H */
