/*
 * phmm_amd_usage.h -- companion of phmm_amd.h: per read, how often the read used every node (or node group) by state,
 * over its mapping lists: a sparse read-by-key matrix.
 *
 * phmm_amd.h's symbol table is closed (the ABI tests pin its entry points one by one); an entry point added
 * after that is declared in a companion header of its own, which includes phmm_amd.h.  The library exports
 * all sets; dbgphmm_amd/_ffi_usage.py lists this header's symbols in USAGE_SYMBOLS and binds them.
 */
#ifndef PHMM_AMD_USAGE_H
#define PHMM_AMD_USAGE_H

#include "phmm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The rows of one phmm_run_with_mapping_read_usage call.  The handle owns its device buffers and borrows nothing: it
 * stays valid after the model, the reads and the mappings are destroyed.  It lives on the device of the call. */
typedef struct phmm_read_usage phmm_read_usage;

/* READ USAGE.  PHMMOutput::to_state_probs() and to_node_freqs() (hmmv2/freq.rs:237-255) of every read on its lists:
 * for ONE read, how often it used each node, by state.  Every usage figure the other calls return (out_node_freq of
 * phmm_generate_mappings, phmm_mappings_node_freqs) is this, summed over the reads.
 *
 * The call runs phmm_run_with_mapping_states (phmm_amd_states.h) with its per-entry values kept on the device and
 * reduces them there; state_logp below is what that call writes for the same inputs and knobs.
 *
 * KEYS.  With n_groups == 0 the key of node v is v, and K = N (the node count).  Otherwise the groups are given as
 * phmm_likelihood_set_groups takes them -- group_off[n_groups + 1], group_nodes[group_off[n_groups]], host pointers,
 * disjoint sets -- the key of v is its group, and K = n_groups.  A node in no group has no key: its list entries are
 * left out.  Empty groups are allowed.
 *
 * ROW of read r: the distinct keys among the entries of r in the mappings' CSR, in ascending order -- the entries
 * row_off[r] .. row_off[r + 1] - 1 of keys[] and usage[][3].  A node listed twice at a position counts twice, as the
 * states call gives each entry its value.
 *   usage[e][s], s = 0 Match, 1 Ins, 2 Del:  the sum of exp(state_logp[a][s]) over the read's entries a with that key;
 *   exp(-inf) is exactly 0.
 * Which keys a row holds is decided by the lists alone: a key whose terms are all 0 stays, with zeros.
 * usage[e][0] + usage[e][1] + usage[e][2] is the reference's to_node_freqs()[v] of that read, the three together its
 * to_state_probs()  (merged index 0 adds nothing: f_init has mass in MatchBegin only).
 *
 *   out_logp_forward[R]    that of the states call, bit for bit;
 *   out_key_usage[K][3]    the column totals over all reads, to_state_probs summed over the read set; a key in no row
 *                          gets 0;
 *   *out                   the rows; out == NULL: scores and totals only.
 *
 * ORDER OF THE SUMS.  Every sum runs in an order that depends on its segment alone; there are no floating-point atomics.
 * A row entry is the sum over a segment: the n entries of one read with one key, in the order of the CSR (position,
 * then place in the list).
 *   n <= 64:  left to right from 0:  ((0 + t_0) + t_1) + ... + t_{n-1};
 *   n >  64:  64 partial sums p_l = ((0 + t_l) + t_{l+64}) + ..., l = 0..63, then six pairwise rounds
 *             p_l <- p_l + p_{l xor d}, d = 32, 16, 8, 4, 2, 1; the result is p_0.
 * A column total is the sum over the segment of one key: its row entries in read order, always by the second rule (for
 * any n).  So a read's row depends on the model, the read and its lists only -- not on the other reads, the capacity
 * class, the chunking under phmm_set_workspace_limit or where the outputs live -- and repeated calls return the same
 * bits.
 *
 * Each output pointer may be NULL, a host pointer or a device pointer.
 * REFUSALS, with nothing written and *out left as it was: those of the states call (NULL model, reads or mappings and
 * mappings of another read set PHMM_EINVAL, a list of more than 400 nodes PHMM_ECAPACITY, node degree above 8, a listed
 * node >= the node count and a read of probability 0 on its lists PHMM_EINVAL); PHMM_ECAPACITY when the states plane
 * (24 bytes per list entry, the whole call) exceeds the workspace limit, as the MEA call refuses; the group refusals of
 * phmm_likelihood_set_groups, all PHMM_EINVAL: offsets not starting at 0 or decreasing, a node id >= N, a node in two
 * groups or twice in one, NULL arrays with n_groups > 0.  Two of this call alone, both PHMM_ECAPACITY: a single read of
 * more than 2^30 list entries, and out_key_usage with more than 2^31 - 2 row entries over all reads.
 * NO READS: no output array is written, and *out is a handle of 0 rows.
 *
 * WORKSPACE.  All scratch comes from the model's device workspace.  Beyond the plane the reduction takes 32 bytes per
 * list entry of a chunk plus the temporary storage of its radix sort (about 12 bytes per entry more): when that does
 * not fit phmm_set_workspace_limit, or a chunk would pass 2^30 entries, the reads run in chunks of consecutive whole
 * reads, one read at the least.  The sort behind out_key_usage is not chunked: about 20 bytes per row entry, which is
 * less than the plane the call holds in any case (a row entry sums at least one list entry).
 * STATISTICS.  Index 2 of phmm_last_call_stats counts the reduction alone -- device time, launches, cells = list
 * entries; the other indices are those of the states half.  The call has no knob of its own: the environment knobs of
 * the states pass act on its states half as documented there. */
int phmm_run_with_mapping_read_usage(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mappings,
                                     uint32_t n_groups, const uint64_t *group_off, const uint32_t *group_nodes,
                                     double *out_logp_forward, double *out_key_usage, phmm_read_usage **out);

/* R, K and the number of row entries over all reads; 0 for a NULL handle */
uint64_t phmm_read_usage_reads(const phmm_read_usage *u);
uint64_t phmm_read_usage_keys(const phmm_read_usage *u);
uint64_t phmm_read_usage_total(const phmm_read_usage *u);

/* row_off[R + 1], keys[total], usage[total][3]; each may be NULL, a host pointer or a device pointer.  A handle of 0
 * rows from a call without reads writes row_off[0] = 0 alone.  PHMM_EINVAL for a NULL handle and for a handle of another
 * device than the current one (phmm_set_device). */
int phmm_read_usage_export(const phmm_read_usage *u, uint64_t *row_off, uint32_t *keys, double *usage);

/* NULL is allowed */
void phmm_read_usage_destroy(phmm_read_usage *u);

#ifdef __cplusplus
}
#endif
#endif /* PHMM_AMD_USAGE_H */
