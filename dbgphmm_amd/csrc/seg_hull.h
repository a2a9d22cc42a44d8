// Segments of the dense backward kernel's run skipping ("Run skipping"): the segment size of a run
// length, and the part of its run that a row walks for a mask of marked segments.  No HIP types: bwd_step (dense.hip)
// and the stand-alone program of tests/test_bwd_skip_segments_cpu.py share these two functions.
#pragma once

#if defined(__HIPCC__)
#define PHMM_SEG_FN __host__ __device__ inline
#else
#define PHMM_SEG_FN inline
#endif

namespace phmm {

static constexpr int SEGS_PER_RUN = 8;  // one bit per segment in a run's byte of A

// A segment is S consecutive node ids, sigma = node / S.  A run of npt nodes holds 8 segments when npt divides by 8,
// otherwise it is its own single segment (masks per run); runs stay aligned with segments either way.
PHMM_SEG_FN int seg_size(int npt) { return npt % SEGS_PER_RUN == 0 ? npt / SEGS_PER_RUN : npt; }

// log2 of the segments a run of npt nodes holds (3 or 0): segment sigma is bit sigma & ((1 << l) - 1) of the byte of
// run sigma >> l.
static constexpr int SEGS_PER_RUN_LOG2 = 3;
static_assert(SEGS_PER_RUN == 1 << SEGS_PER_RUN_LOG2, "a run's byte of A holds one bit per segment");
PHMM_SEG_FN int segs_per_run_log2(int npt) { return npt % SEGS_PER_RUN == 0 ? SEGS_PER_RUN_LOG2 : 0; }

// mask: bit s = segment s of the run is marked (bits 0..7).  jtop: the run's top row, 0-based from the run's first
// node (npt - 1, or less in the last run of the column).  False: nothing is marked, the row walks nothing.  Otherwise
// the row walks the hull of the marked segments: nodes first .. first + top of the run, top >= 0 (a marked segment
// starts at a node of the column).
PHMM_SEG_FN bool seg_hull(unsigned mask, int S, int jtop, int *first, int *top) {
    if (!mask) return false;
    const int lo = __builtin_ctz(mask), hi = 31 - __builtin_clz(mask);
    const int t = hi * S + S - 1;
    *first = lo * S;
    *top = (t < jtop ? t : jtop) - lo * S;
    return true;
}

}  // namespace phmm
