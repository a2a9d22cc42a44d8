/*
 * phmm_amd_share.h -- companion of phmm_amd.h: what the dense head shared between reads with equal prefixes.
 *
 * phmm_amd.h's symbol table is closed (the ABI tests pin its entry points one by one); an entry point added
 * after that is declared in a companion header of its own, which includes phmm_amd.h.  The library exports
 * all sets; dbgphmm_amd/_ffi.py lists this header's symbols in EXTENSION_SYMBOLS.
 */
#ifndef PHMM_AMD_SHARE_H
#define PHMM_AMD_SHARE_H

#include "phmm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Column j of a read's dense forward table depends on the model and on the read's bases 0..j alone, so the adaptive
 * calls (phmm_full_prob_reads and phmm_generate_mappings without mappings, use_max_ratio) compute the first J columns
 * of their main plan once per distinct prefix, on 4^J virtual reads, and every read takes them from there.  Results
 * are the bits of the unshared path; phmm_reads_last_call_info and the grouping hints are unchanged.
 *
 *   out_columns        J of this thread's most recent such call: 0 when sharing was off, not worth it (few read
 *                      groups), or declined -- a read shorter than J + 2 bases, a base among a read's first J that is
 *                      none of the (at most four) codes the model emits, J + 2 beyond n_warmup or the kept columns, a
 *                      read-group width below 64, or a prefix that leaves the dense warm-up before column J;
 *   out_virtual_lanes  4^J, the virtual reads walked; 0 with J = 0.
 *
 * Either pointer may be NULL.  Always PHMM_OK; a read-only getter, no device needed.
 * Developer knob PHMM_SHARE_PREFIX: unset = the planner's J (2..6, by the read groups and the memory), 0 = off,
 * 1..6 = that J wherever the plan is eligible.  phmm_last_call_stats(0) counts the cells walked: the virtual plan's and
 * the reads' own from column J on. */
int phmm_last_call_prefix_share(int *out_columns, uint64_t *out_virtual_lanes);

#ifdef __cplusplus
}
#endif
#endif /* PHMM_AMD_SHARE_H */
