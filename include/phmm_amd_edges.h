/*
 * phmm_amd_edges.h -- companion of phmm_amd.h: per read, how often the read crossed every edge (or key of a caller's
 * edge map) over its mapping lists: a sparse read-by-key matrix.
 *
 * phmm_amd.h's symbol table is closed (the ABI tests pin its entry points one by one); an entry point added
 * after that is declared in a companion header of its own, which includes phmm_amd.h.  The library exports
 * all sets; dbgphmm_amd/_ffi_edges.py lists this header's symbols in EDGES_SYMBOLS and binds them.
 */
#ifndef PHMM_AMD_EDGES_H
#define PHMM_AMD_EDGES_H

#include "phmm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The rows of one phmm_run_with_mapping_read_edges call.  The handle owns its device buffers and borrows nothing: it
 * stays valid after the model, the reads and the mappings are destroyed.  It lives on the device of the call. */
typedef struct phmm_read_edges phmm_read_edges;

/* in edge_key / init_key: the term has no key and is left out */
#define PHMM_NO_KEY 0xffffffffu

/* READ EDGES.  PHMMOutput::to_edge_and_init_freqs() (hmmv2/freq.rs:276-298) of every read on its lists: for ONE read,
 * which transitions of the graph it crossed and how often.  out_edge_freq / out_init_freq of
 * phmm_run_with_mapping_edges are this, summed over the reads.
 *
 * The call runs the list pass of phmm_run_with_mapping_edges -- the same kernels under the same knobs -- and keeps the
 * read of every term where that call sums over the reads.  The pass records, per read position, the nonzero terms of
 * the merged index it holds as (key, value) pairs; the key is the edge id e, or E + v for the Begin -> v transition.
 *
 * KEYS.  With n_keys == 0 the key of edge e is e, the key of Begin -> v is E + v, and K = E + N: the keys the pass
 * writes.  Otherwise K = n_keys, and edge_key[E] and init_key[N] are host arrays of values < n_keys or PHMM_NO_KEY,
 * which leaves the term out.  Either array may be NULL, which leaves every term of that kind out.  Several edges (and
 * Begin transitions) may share a key: their terms add.  (link_keys of the Python package builds the map "ordered pair
 * of unitigs -> key".)
 *
 * ROW of read r: the distinct keys among the nonzero terms the pass records for r, in ascending order -- the entries
 * row_off[r] .. row_off[r + 1] - 1 of keys[] and usage[].
 *   usage[e]:  the sum of those terms: the six transition kinds of to_edge_and_init_freqs summed, as
 *              phmm_run_dense_edges defines out_edge_freq / out_init_freq.
 * A key all of whose terms are exactly 0 is NOT recorded by the pass and is not in the row: which keys a row holds is
 * decided by the values.  (This differs from phmm_run_with_mapping_read_usage, where the lists alone decide the keys
 * and a key of zero terms stays, with zeros.)  A key absent from the row counts as 0.
 *
 * END TERMS.  B's initial table has m = d = p_end on every node, so every read has Begin terms on ALL N nodes at its
 * last base.  They are not recorded and are not row entries; they come from two scalars per read,
 * out_end_terms[r][0] = A_r and out_end_terms[r][1] = T_r:
 *   init_freq_r[v] = (usage at key E + v in row r, 0 if absent) + init_v * (A_r + T_r * e_v(x_last)),
 * init_v the initial probability of node v, x_last the read's last base, e_v(x) = p_match where x is the emission of v
 * and p_mismatch otherwise.  With L the read's length, P its probability (exp of out_logp_forward[r]), ib_j the
 * forward InsBegin chain of the model (ib_0 = p_random * p_MI, ib_j = p_random * p_II * ib_{j-1}; kept as logs) and c_M
 * the coefficient of the step from InsBegin into Match:
 *   A_r = p_ID * p_end * ib_{L-1} / P                      (merged index L, Begin -> Del of v)
 *   T_r = c_M * p_end * ib_{L-2} / P,  c_M = p_IM          (merged index L-1, Begin -> Match of v, L >= 2)
 *   T_r = p_MM * p_end / P                                 (the one-base read, L == 1: mb = 1, c_M(0) = p_MM, ib_{-1} = 1)
 * both evaluated as coefficient * p_end * exp(ln ib - ln P).
 *
 *   out_logp_forward[R]    that of phmm_run_with_mapping_edges, bit for bit;
 *   out_end_terms[R][2]    (A_r, T_r) above;
 *   out_key_usage[K]       the column totals of the rows over all reads, the end terms excluded; a key in no row gets
 *                          0.  With the default keys out_key_usage[0..E) is out_edge_freq of
 *                          phmm_run_with_mapping_edges and out_key_usage[E + v] + init_v * sum_r (A_r + T_r
 *                          e_v(x_last of r)) its out_init_freq[v], both up to the order of the sums;
 *   *out                   the rows; out == NULL: scores and totals only.
 *
 * ORDER OF THE SUMS.  Every sum runs in an order that depends on its segment alone; there are no floating-point atomics.
 * A row entry is the sum over a segment: the n records of one read with one key, in record order (position, then the
 * order in which the kernel appended them to the position's record).
 *   n <= 64:  left to right from 0:  ((0 + t_0) + t_1) + ... + t_{n-1};
 *   n >  64:  64 partial sums p_l = ((0 + t_l) + t_{l+64}) + ..., l = 0..63, then six pairwise rounds
 *             p_l <- p_l + p_{l xor d}, d = 32, 16, 8, 4, 2, 1; the result is p_0.
 * A column total is the sum over the segment of one key: its row entries in read order, always by the second rule (for
 * any n).
 * BITS.  A read's row depends on the model, the read, its lists and the knobs in force only -- not on the other reads of
 * the call, on where the outputs live or on earlier calls -- and repeated calls return the same bits.  Across the
 * kernel classes of the pass (the 64-slot and the 400-slot wave kernels, the opt-in block under PHMM_WIDE_HINTED with
 * PHMM_WIDE_EDGE_BWD) the rows agree to rounding only: the order in which a class appends the terms of one position is
 * its own.  A read's class follows from its longest list and the knobs.
 *
 * Each output pointer may be NULL, a host pointer or a device pointer.
 * REFUSALS, with nothing written and *out left as it was: those of phmm_run_with_mapping_edges (NULL model, reads or
 * mappings and mappings of another read set PHMM_EINVAL, a list of more than 400 nodes PHMM_ECAPACITY, node degree
 * above 8, a listed node >= the node count, and a read of probability 0 on its lists PHMM_EINVAL naming the read); the
 * key-map refusals, PHMM_EINVAL: n_keys > 0 with edge_key and init_key both NULL, a value >= n_keys that is not
 * PHMM_NO_KEY, n_keys == PHMM_NO_KEY; PHMM_ECAPACITY for more than 2^31 - 2 records or row entries (the sorts count in
 * int), and when the reduction's scratch exceeds the workspace limit (below).
 * NO READS: no output array is written, and *out is a handle of 0 rows.
 *
 * WORKSPACE.  All scratch comes from the model's device workspace and goes back when the call ends, as that of
 * phmm_run_with_mapping_edges does: from the second identical call on phmm_workspace_bytes() does not change.  Beyond
 * the list pass the reduction takes 32 bytes per record plus the temporary storage of its radix sort (about 12 bytes
 * per record more).  The reduction is NOT chunked (nor is the record stream of the pass): when its scratch exceeds
 * phmm_set_workspace_limit the call refuses with PHMM_ECAPACITY; call it on fewer reads.
 * STATISTICS.  Index 2 of phmm_last_call_stats counts the reduction alone -- device time, launches, cells = records
 * reduced; the other indices are those of phmm_run_with_mapping_edges (index 4: the block class).  The call has no
 * knob of its own. */
int phmm_run_with_mapping_read_edges(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mappings,
                                     uint32_t n_keys, const uint32_t *edge_key, const uint32_t *init_key,
                                     double *out_logp_forward, double *out_end_terms, double *out_key_usage,
                                     phmm_read_edges **out);

/* R, K and the number of row entries over all reads; 0 for a NULL handle */
uint64_t phmm_read_edges_reads(const phmm_read_edges *u);
uint64_t phmm_read_edges_keys(const phmm_read_edges *u);
uint64_t phmm_read_edges_total(const phmm_read_edges *u);

/* row_off[R + 1], keys[total], usage[total]; each may be NULL, a host pointer or a device pointer.  A handle of 0
 * rows from a call without reads writes row_off[0] = 0 alone.  PHMM_EINVAL for a NULL handle and for a handle of another
 * device than the current one (phmm_set_device). */
int phmm_read_edges_export(const phmm_read_edges *u, uint64_t *row_off, uint32_t *keys, double *usage);

/* NULL is allowed */
void phmm_read_edges_destroy(phmm_read_edges *u);

#ifdef __cplusplus
}
#endif
#endif /* PHMM_AMD_EDGES_H */
