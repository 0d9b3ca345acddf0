// mpdata_convert.h -- host interface of the first-order conversion between two tracers of f, in place (mpdata_convert.hip;
// include/mpdata_hip.h 3t): per instance sl of the block (b = sl - sl0), level k = 1 .. nlev and INTERIOR column
// i = 1 .. nx, with a = f_old(i,k,src) and c = f_old(i,k,dst), every statement rounded once in the arrays' precision, in
// this association, no contraction, comparisons plain compare-and-select:
//   r(b,k) == 0   :  the level keeps every bit in BOTH tracers and is not stored; dsum(b,k) = +0
//   e = q0 ? a - q0(b,k) : a;   e = (e > 0) ? e : +0;   d = r(b,k) * e
//   limit         :  m = (a > 0) ? a : +0;   d = (d > m) ? m : d
//   f(i,k,src) = a - d;   g = y ? y(b,k) * d : d;   f(i,k,dst) = c + g
//   dsum(b,k)     :  s = +0; do i = 1, nx: s = s + d(i)                          (NULL: skipped)
// r, q0, y, dsum (n, nlev): reference layout, leading dimension n, the block's first instance at index 0.  r, q0 and y are
// only read, and nothing outside the arrays is touched; halo columns and every other tracer are neither read nor written.
#ifndef MPDATA_CONVERT_H
#define MPDATA_CONVERT_H
#include <hip/hip_runtime.h>

#include "mpdata_wm_walk.h"

// Plan layout.  j: the plan side of f exactly as wm_job(which = 0) makes it for ALL tracers of the plan (j.prv on tracer
// 0, strides in 8-byte elements; j.ref is not used); src != dst, both in [0, j.ntr).
//   The grid runs over (tile, 64-element slice) of the tiles the block touches -- no tracer axis.  A lane owns one
//   element and walks its interior column slots (mpdata_wm_walk.h) as TWO linear streams, NB columns in flight on each:
//   the src stream at j.prv + src * prv_tstride, the dst stream at the signed 64-bit offset (dst - src) * prv_tstride
//   from it (dst < src: a negative offset).  r, q0, y of the lane's instance and level are in registers per half, loaded
//   once; dsum is lane-local, accumulated in column order.  No LDS, no barrier: a lane touches the columns of its own
//   element only, in two tracers.
//   sel: the block (mpdata_wm_walk.h).  A slot that is no instance of it keeps its bits (the partner half of a split
//     pair is stored back as it was loaded; a lane none of whose halves is in the block stores nothing).  The PHANTOM of
//     an odd fp32 plan takes the result of the plan's last slot, its partner in the pair, in BOTH tracers, whenever the
//     block holds that instance and its r is not zero on that level (W > 1: the kernel leaves the inner plan's phantom
//     alone and the caller restores it behind the call).
//     W > 1 (windowed plans): only the levels a window OWNS are read and written, each with r, q0 and y of the tall
//     level it stands for; dsum is written by each level's owner.  The caller need not refresh the seams in front, and
//     marks them stale afterwards.
struct MpdataConvertJob {
  MpdataLayoutJob j;
  MpdataBlockSel sel;
  int src, dst;
  const void* r;
  const void* q0;   // NULL: no threshold
  const void* y;    // NULL: yield 1, no multiply
  int limit;        // != 0: d is capped from above by max(a, 0)
  void* dsum;       // NULL: not wanted
};
hipError_t mpdata_convert_wm(const MpdataConvertJob& b, hipStream_t stream);

// Reference layout: f(ld, -2:nx+3, nlev, ntr) with elem_bytes = 4 or 8, instances [sl0, sl0 + n) of its ld.  One thread
// per instance and level row, one loop over i, 64-bit offsets (the dst row at a signed offset from the src row), in
// place: a thread reads and writes its own row of the two tracers only.
hipError_t mpdata_convert_ref(void* f, int elem_bytes, long long ld, long long sl0, long long n, int nx, int nlev, int ntr, int src,
                              int dst, const void* r, const void* q0, const void* y, int limit, void* dsum, hipStream_t stream);

#endif
