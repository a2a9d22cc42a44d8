/*
 * phmm_amd_align.h -- companion of phmm_amd.h: the best path or S sampled paths of every read over its mapping lists
 * as self-contained alignment records, a CIGAR and a node walk each, built on the device from rows that never leave it.
 *
 * phmm_amd.h's symbol table is closed (the ABI tests pin its entry points one by one); an entry point added
 * after that is declared in a companion header of its own, which includes phmm_amd.h.  The library exports
 * all sets; dbgphmm_amd/_ffi_align.py lists this header's symbols in ALIGN_SYMBOLS and binds them.
 */
#ifndef PHMM_AMD_ALIGN_H
#define PHMM_AMD_ALIGN_H

#include "phmm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the op of an event; the values are BAM's */
#define PHMM_ALN_INS  1 /* Ins on a node, or InsBegin */
#define PHMM_ALN_DEL  2 /* Del */
#define PHMM_ALN_EQ   7 /* Match on a node whose emission equals the read's base */
#define PHMM_ALN_DIFF 8 /* Match on a node whose emission differs */

/* THE RECORD.  A path, as phmm_amd_path.h defines it, is a sequence of EVENTS: for base p = 0 .. L-1 the emitting state
 * of p, then the Del states behind it, in order (the entries of row p of out_path up to its padding).  Every event has
 * an op: PHMM_ALN_EQ / PHMM_ALN_DIFF for a Match, decided as out_counts[0] and out_counts[1] decide it (the emission of
 * the node against x_p), PHMM_ALN_INS for Ins and InsBegin, PHMM_ALN_DEL for Del.  Match and Del events are STEPS; the
 * step's node is nodes[pos_off[g] + slot] of the input CSR.  Ins and InsBegin are no steps.
 *   CIGAR  the maximal runs of equal ops over the events, in order; one uint32 per run, (len << 4) | op.
 *   WALK   the maximal runs over the steps, in order, in which each step's node id is the previous step's node id plus
 *          one; one pair (run_node, run_len) of uint32 per run, run_node the first node of the run.  A self-loop taken
 *          twice is two runs of length 1; a graph numbered against its unitigs gives runs of length 1.  The record is
 *          lossless under any numbering and short under one that follows the unitigs.
 * A read with no path (ln P = -inf) and an empty read have 0 CIGAR words and 0 walk runs.
 *
 * INVARIANTS of every alignment:  the lengths of =, X and I sum to L;  the four op totals equal out_counts[..][0..3]
 * (=, X, I, D);  the walk's run lengths sum to the total of =, X and D.
 *
 * LOSSLESS.  The record determines the (node, kind) sequence of the path: an I before the first step is InsBegin, an I
 * after a step sits on the last step's node, and =, X and D consume one step each (= and X are Match, D is Del).
 *
 * ALIGNMENT INDEX.  a = r * S' + s with S' = max(n_samples, 1): read-major, a read's samples are contiguous.
 *
 *   n_samples == 0      the best path of phmm_amd_path.h (seed is ignored, out_path_logp is not written);
 *   n_samples 1..64     exactly the walks phmm_run_with_mapping_sample_paths draws for (seed, r, s);
 *   out_logp[R]         the best ln P, or ln Z;
 *   out_path_logp[R][S] ln P of each sampled path;
 *   out_counts[R][S'][4]  =, X, I, D of each alignment;
 *   *out                the records, a handle that owns its device buffers and borrows nothing once the call has
 *                       returned: the model, the reads and the mappings may be destroyed before it.
 *
 * Every output pointer may be NULL, a host pointer or a device pointer; out == NULL gives scores and counts only.
 * Refusals are those of phmm_run_with_mapping_best_path and phmm_run_with_mapping_sample_paths (n_samples >
 * PHMM_SAMPLE_MAX included), with nothing written and *out left as it was.  No reads: no output array is written and
 * *out is a handle of 0 alignments.  A read's record depends on the model, the read, its lists and, for samples, on
 * seed, r and s alone: not on the other reads, the capacity class, chunking under phmm_set_workspace_limit or where the
 * outputs live; repeated calls return the same bits.  The rows are staged in the device workspace chunk by chunk, as
 * for a host out_path of the parent calls, and compacted there; a record never crosses a chunk.  A run length is held
 * in 28 bits: reads of 2^28 events and more are not supported.  Index 2 of phmm_last_call_stats counts the call's device
 * time, launches (two more per chunk than the parent call) and cells (list entries).  The call has no knob. */
typedef struct phmm_alignments phmm_alignments;

int phmm_run_with_mapping_alignments(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mappings,
                                     uint32_t n_samples, uint64_t seed,
                                     double *out_logp, double *out_path_logp, uint32_t *out_counts,
                                     phmm_alignments **out);

uint64_t phmm_alignments_count(const phmm_alignments *a);      /* R * S' */
uint64_t phmm_alignments_total_ops(const phmm_alignments *a);  /* CIGAR words */
uint64_t phmm_alignments_total_runs(const phmm_alignments *a); /* walk runs */
/* op_off[A + 1] and run_off[A + 1]: the words of alignment a are ops[op_off[a] .. op_off[a + 1]) and its runs
 * run_node / run_len[run_off[a] .. run_off[a + 1]).  Each pointer may be NULL, a host or a device pointer.  The calling
 * thread's device must be the one the handle was made on. */
int phmm_alignments_export(const phmm_alignments *a, uint64_t *op_off, uint32_t *ops,
                           uint64_t *run_off, uint32_t *run_node, uint32_t *run_len);
void phmm_alignments_destroy(phmm_alignments *a);

#ifdef __cplusplus
}
#endif
#endif /* PHMM_AMD_ALIGN_H */
