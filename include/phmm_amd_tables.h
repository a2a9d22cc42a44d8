/*
 * phmm_amd_tables.h -- companion of phmm_amd.h: the forward and backward tables of the list pass themselves, per
 * list entry and per base.
 *
 * phmm_amd.h's symbol table is closed (the ABI tests pin its entry points one by one); an entry point added
 * after that is declared in a companion header of its own, which includes phmm_amd.h.  The library exports
 * all sets; dbgphmm_amd/_ffi_tables.py lists this header's symbol in TABLES_SYMBOLS and binds it.
 */
#ifndef PHMM_AMD_TABLES_H
#define PHMM_AMD_TABLES_H

#include "phmm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* PHMMModel::forward_with_mapping (forward.rs:51-75) and backward_with_mapping (backward.rs:59-93) of every read on its
 * lists, returned as the PHMMTables they are: what bin/mapping.rs and bin/table.rs print base by base.  phmm_dense_tables
 * and phmm_backward_sparse_tables do this for the dense and the adaptive drivers; this call does it for the list drivers.
 *
 * Indexing is that of phmm_amd_states.h: read r of length L, position p in 0..L-1, global position
 * g = read_off[r] + p; entry a runs over [pos_off[g], pos_off[g+1]) of the INPUT mappings, v = nodes[a].  All values are
 * natural logs, -inf for a probability of 0.
 *   out_forward[total_entries][3]        [3a + s], s = 0, 1, 2: ln F.tables[p].{m, i, d}[v];
 *   out_forward_scalars[total_bases][2]  [2g + 0] = ln F.tables[p].ib, [2g + 1] = ln F.tables[p].e: e is the likelihood of
 *                                        the prefix ending at base p.  F.tables[p].mb is 0 for every p (fmb,
 *                                        forward.rs:531-533) and is not returned;
 *   out_backward[total_entries][3]       ln B.tables[p].{m, i, d}[v].  THE MERGED INDEX: this is the table that lives on
 *                                        list p, B.tables[p]; it is NOT B.table_merged(p + 1), the table that
 *                                        phmm_run_with_mapping_states multiplies F.tables[p] with (table.rs:414-434:
 *                                        merged index i is F.tables[i - 1] and B.tables[i]);
 *   out_backward_scalars[total_bases][2] [2g + 0] = ln B.tables[p].mb, [2g + 1] = ln B.tables[p].ib: mb is the likelihood
 *                                        of the suffix from base p.  B.tables[p].e is 0 (be, backward.rs:563-565) and is
 *                                        not returned;
 *   out_logp_forward[R]                  ln F.tables[L-1].e;
 *   out_logp_backward[R]                 ln B.tables[0].mb.
 * Each per-read total carries the same bits as the matching scalar of the same call.  F.ib * B.table_merged(p + 1).ib / P
 * is the posterior that base p was emitted from InsBegin.
 *
 * The two tables at the ends are constants of the parameters and are not returned: f_init = F.table_merged(0) has mb = 1
 * and 0 everywhere else (forward.rs:255-266); b_init = B.table_merged(L) has m = i = d = p_end at every node and
 * mb = ib = e = 0 (backward.rs:197-211).
 *
 * Any output may be NULL, a host pointer or a device pointer.  A half (forward or backward) none of whose outputs is asked
 * for is not run.
 * Refusals are those of phmm_run_with_mapping_edges, with nothing computed: NULL model, reads or mappings and mappings of
 * another read set PHMM_EINVAL, a list of more than 400 nodes PHMM_ECAPACITY, node degree above 8 PHMM_EINVAL.  A list
 * that names a node twice is PHMM_EINVAL as well, found on the device: the outputs are then unspecified.
 * A read whose probability on its lists is 0 is a result, not a refusal (as in phmm_run_with_mapping_best_path): its
 * values are -inf from where the mass ends.  An empty list gives e = -inf at that position, and the InsBegin chain
 * carries on behind it, as in the reference.  No reads: nothing is written.
 * Precision.  A column is kept as values times one power of two, so a value more than about 1e-300 below the largest of
 * its column (entries and InsBegin) may come back as -inf.  A read on which the forward pass notices that this loses what
 * matters -- the read of a model that cuts its path, whose probability re-enters from the InsBegin chain -- is computed
 * again with an exponent per value.
 * Host outputs are staged in the device workspace (48 bytes per list entry and 32 per base when everything is asked for)
 * and given back when the call ends; under phmm_set_workspace_limit the reads run in chunks of consecutive reads.  A
 * read's outputs depend on the read and its lists alone; repeated calls return the same bits.  The call honours
 * phmm_set_stream.  Index 2 of phmm_last_call_stats counts the call's device time, launches and cells (list entries). */
int phmm_run_with_mapping_tables(phmm_model *m, const phmm_reads *reads, const phmm_mappings *mappings,
                                 double *out_logp_forward, double *out_logp_backward,
                                 double *out_forward, double *out_forward_scalars,
                                 double *out_backward, double *out_backward_scalars);

#ifdef __cplusplus
}
#endif
#endif /* PHMM_AMD_TABLES_H */
