// mpdata_column_cond.h -- host interface of the per-column conditional level counts, tops and paths of the tracers of f
// (mpdata_column_cond.hip; include/mpdata_hip.h 3w): the transposed twin of mpdata_level_cond.h, as mpdata_column_path.h is
// of the level statistics.  Per instance sl of the block (b = sl - sl0) and INTERIOR column i = 1 .. nx, along the levels
// k = 1 .. nlev, with c_k = f(sl,i,k,tc) and v_k = f(sl,i,k,t), every statement rounded once in the arrays' precision, in
// this association, no contraction, the comparisons plain compare-and-select:
//   wgt(sl,k)    = rho(sl,k) * adz(sl,k)
//   in_k         = (lo ? c_k >  lo(b,k) : true)  and  (hi ? c_k <= hi(b,k) : true)
//   kcnt(b,i)    :  q = +0;  do k = 1, nlev:  if in_k:  q = q + 1
//   kbot(b,i)    :  the smallest k with in_k as a real, +0 if there is none;   ktop(b,i): the largest
//   cpath(b,i,j) :  s = +0;  do k = 1, nlev:  if in_k:  s = s + wgt(sl,k) * v_k      (j = t - first, t in [first, first + ntr))
//   cover(b)     :  q = +0;  do i = 1, nx:  if kcnt(b,i) > 0:  q = q + 1            (a second kernel, from kcnt)
//   mass(b,j)    :  s = +0;  do i = 1, nx:  s = s + cpath(b,i,j)                     (a second kernel, from cpath)
// A level that is not in is SELECTED away, never multiplied away: whatever an excluded cell of a value tracer holds -- an
// infinity, a NaN -- does not reach cpath.  lo, hi (n, nlev), kcnt, kbot, ktop (n, nx), cpath (n, nx, ntr), cover (n), mass
// (n, ntr): reference layout, leading dimension n, the block's first instance at index 0.  f, rho, adz, lo and hi are only
// read and nothing outside the outputs is written; halo columns and the tracers outside tc and the range are not read.
#ifndef MPDATA_COLUMN_COND_H
#define MPDATA_COLUMN_COND_H
#include <hip/hip_runtime.h>

#include "mpdata_wm_walk.h"

// Plan layout.  j: the plan side of f exactly as wm_job(which = 0) makes it for ALL tracers of the plan (j.prv on tracer
// 0, strides in 8-byte elements; j.ref is not used); tc in [0, j.ntr), [first, first + ntr) inside it (ntr = 0 with a
// NULL cpath).  rho, adz, kc_tile_stride: as in MpdataColumnPathJob.
//   The grid runs over (group of units, batch of columns) as col_groups_batched makes them with three coefficient rows
//   -- no tracer axis: the value tracers are a loop inside the kernel.  Per window a workgroup stages the tc columns of
//   its group and batch through LDS as linear streams (the staging of mpdata_column_path.hip) with the rows wgt, lo and
//   hi; a lane per (unit, column) walks its levels in rising order, keeps the in-bits of its levels in registers (eight
//   32-bit words per half, two for a window; the words rotate through position 0, so no register is indexed at run
//   time) and forms kcnt, kbot, ktop from them with integer bit counts.  Then every value tracer is staged into the
//   same columns of LDS and summed under those bits: the condition is staged and compared once.  W = 1: a tracer's sum
//   is stored behind its walk, any number of tracers share the condition.  W > 1: the running sums of up to eight
//   tracers (CC_TCH) stay in registers across the windows; a ninth tracer starts a second pass.  Every load of a
//   batch comes before a barrier, every reuse of LDS behind one; no lane talks to another.  The kernel copies its
//   arguments to the head of its LDS once and reads addresses and strides from there, and it is built per given bound
//   (lo, hi, both): the scalar registers hold the loop nest without a spill.
//   sel: the block (mpdata_wm_walk.h).  A slot that is no instance of it -- padding, the phantom half of an odd fp32 plan,
//     the partner of a split pair, a neighbour in the group -- reaches no output.
//     W > 1 (windowed plans): the windows are staged one after the other, only the levels a window OWNS are read, each
//     with lo, hi and the weight of the tall level it stands for, in rising order of the tall level; kbot and ktop are
//     tall levels; the running values stay in registers.  The caller need not refresh the seams in front.
struct MpdataColumnCondJob {
  MpdataLayoutJob j;
  const void *rho, *adz;
  long long kc_tile_stride;
  MpdataBlockSel sel;
  int tc;           // the condition tracer
  int first, ntr;   // the value tracers (cpath NULL: not looked at)
  const void* lo;   // NULL: no lower bound
  const void* hi;   // NULL: no upper bound (one of the two is given)
  void *kcnt, *kbot, *ktop, *cpath;   // NULL: not wanted (one of the six is given)
  void *cover, *mass;                 // cover needs kcnt, mass needs cpath
};
hipError_t mpdata_column_cond_wm(const MpdataColumnCondJob& b, hipStream_t stream);

// Reference layout: f(ld, -2:nx+3, nlev, ntr_all), rho(ld, nlev), adz(ld, nlev) with elem_bytes = 4 or 8, instances
// [sl0, sl0 + n) of their ld.  One thread per instance and column, the loops over k and the value tracers inside, 64-bit
// offsets (a value tracer's column at a signed offset from the tc column; the comparison is made again per tracer).
hipError_t mpdata_column_cond_ref(const void* f, const void* rho, const void* adz, int elem_bytes, long long ld, long long sl0,
                                  long long n, int nx, int nlev, int ntr_all, int tc, const void* lo, const void* hi, void* kcnt,
                                  void* kbot, void* ktop, void* cpath, void* cover, void* mass, int first, int ntr, hipStream_t stream);

#endif
