// mpdata_level_cov.h -- host interface of the per-level covariance of two tracers of f (mpdata_level_cov.hip;
// include/mpdata_hip.h 3u): per instance sl of the block (b = sl - sl0), level k = 1 .. nlev, over the INTERIOR columns
// i = 1 .. nx, with a_i = f(i,k,ta) and b_i = f(i,k,tb), every statement rounded once in the arrays' precision, in this
// association, no contraction, the divide the correctly rounded IEEE one:
//   raw       :  da_i = a_i ;  db_i = b_i                                        (no subtraction at all)
//   otherwise :  m_a = ma ? ma(b,k) : ( s = +0; do i = 1, nx: s = s + a_i ;  s / nx )
//                m_b = mb ? mb(b,k) : the same from b_i
//                mean_a(b,k) = m_a ;  mean_b(b,k) = m_b                          (NULL: skipped; written in both cases)
//                da_i = a_i - m_a ;  db_i = b_i - m_b
//   c = +0;  do i = 1, nx:  p = da_i * db_i ;  c = c + p ;   cov(b,k) = c         (the SUM: the caller normalises)
// ma, mb, cov, mean_a, mean_b (n, nlev): reference layout, leading dimension n, the block's first instance at index 0.  f,
// ma and mb are only read, and nothing outside the three outputs is written; halo columns and every other tracer are not
// read.  ta == tb is allowed (the variance; ma and mb may still differ).
#ifndef MPDATA_LEVEL_COV_H
#define MPDATA_LEVEL_COV_H
#include <hip/hip_runtime.h>

#include "mpdata_wm_walk.h"

// Plan layout.  j: the plan side of f exactly as wm_job(which = 0) makes it for ALL tracers of the plan (j.prv on tracer
// 0, strides in 8-byte elements; j.ref is not used); ta, tb in [0, j.ntr).
//   The grid runs over (tile, 64-element slice) of the tiles the block touches -- no tracer axis.  A lane owns one
//   element and walks its interior column slots (mpdata_wm_walk.h) as TWO linear streams, NB columns in flight on each:
//   the ta stream at j.prv + ta * prv_tstride, the tb stream at the signed 64-bit offset (tb - ta) * prv_tstride from it
//   (tb < ta: a negative offset); with ta == tb it walks ONE stream.  The means and c are lane-local, in column order.  No
//   LDS, no barrier, no cross-lane traffic.  Which form serves which case (all give the same bits):
//     ONE-PASS  raw, or ma and mb both given: nothing is to be summed; one walk.
//     KEPT      a mean is to be formed and nx <= 32 (KEPT_NX1 for ta == tb, KEPT_NX2 for ta != tb, both 32): the columns
//               stay in registers between the summing pass and the accumulating pass, so f is read once (64 registers of
//               data at nx = 32 for one stream, 128 for two: 82 VGPRs and 5 waves per SIMD, and 146 fp64 / 206 fp32 VGPRs
//               and 3 / 2 waves, no scratch, no spill).  Timed against RE-READ at nx = 32 it is 27 % to 33 % faster in
//               both precisions, for one stream and for two, at 28 and at 300 levels (docs/EXPERIMENTS.md AE), so the
//               two-stream limit stays at 32 as well.
//     RE-READ   a mean is to be formed, every other nx: the summing walk of mpdata_stats.hip over the stream or streams
//               that need a mean, the divide or divides, then the accumulating walk over the same columns.
//   sel: the block (mpdata_wm_walk.h).  A slot that is no instance of it -- padding, the phantom half of an odd fp32 plan,
//     the partner of a split pair, a neighbour in the tile -- reaches no output; a wave none of whose elements is in the
//     block (or owned, W > 1) loads nothing.
//     W > 1 (windowed plans): only the levels a window OWNS are read, each with ma / mb of the tall level it stands for,
//     and each is written to that tall level.  The caller need not refresh the seams in front.
struct MpdataLevelCovJob {
  MpdataLayoutJob j;
  MpdataBlockSel sel;
  int ta, tb;
  const void* ma;   // NULL: the mean of the ta row is formed (raw: must be NULL)
  const void* mb;   // NULL: the mean of the tb row is formed (raw: must be NULL)
  int raw;          // != 0: da = a, db = b
  void* cov;
  void* mean_a;     // NULL: not wanted (raw: must be NULL)
  void* mean_b;
};
hipError_t mpdata_level_cov_wm(const MpdataLevelCovJob& b, hipStream_t stream);

// Reference layout: f(ld, -2:nx+3, nlev, ntr) with elem_bytes = 4 or 8, instances [sl0, sl0 + n) of its ld.  One thread
// per instance and level row, loops over i, 64-bit offsets (the tb row at a signed offset from the ta row): the one-pass
// walk, or the summing walk, the divides and the accumulating walk.
hipError_t mpdata_level_cov_ref(const void* f, int elem_bytes, long long ld, long long sl0, long long n, int nx, int nlev, int ntr,
                                int ta, int tb, const void* ma, const void* mb, int raw, void* cov, void* mean_a, void* mean_b,
                                hipStream_t stream);

#endif
