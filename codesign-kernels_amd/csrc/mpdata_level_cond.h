// mpdata_level_cond.h -- host interface of the per-level conditional counts and sums of the tracers of f
// (mpdata_level_cond.hip; include/mpdata_hip.h 3v): per instance sl of the block (b = sl - sl0), level k = 1 .. nlev, over
// the INTERIOR columns i = 1 .. nx, with c_i = f(i,k,tc) and v_i = f(i,k,t), every statement rounded once in the arrays'
// precision, in this association, no contraction, the comparisons plain compare-and-select:
//   in_i = (lo ? c_i >  lo(b,k) : true)  and  (hi ? c_i <= hi(b,k) : true)
//   cnt(b,k)    :  q = +0;  do i = 1, nx:  if in_i:  q = q + 1
//   csum(b,k,j) :  s = +0;  do i = 1, nx:  if in_i:  s = s + v_i          (j = t - first, t in [first, first + ntr))
// A column that is not in is SELECTED away, never multiplied away: whatever an excluded cell of a value tracer holds -- an
// infinity, a NaN -- does not reach csum.  lo, hi, cnt (n, nlev) and csum (n, nlev, ntr): reference layout, leading
// dimension n, the block's first instance at index 0.  f, lo and hi are only read and nothing outside cnt and csum is
// written; halo columns and the tracers outside tc and the range are not read.  tc may lie inside the range.
#ifndef MPDATA_LEVEL_COND_H
#define MPDATA_LEVEL_COND_H
#include <hip/hip_runtime.h>

#include "mpdata_wm_walk.h"

// Plan layout.  j: the plan side of f exactly as wm_job(which = 0) makes it for ALL tracers of the plan (j.prv on tracer
// 0, strides in 8-byte elements; j.ref is not used); tc in [0, j.ntr), [first, first + ntr) inside it (ntr = 0 with a
// NULL csum).
//   The grid runs over (tile, 64-element slice) of the tiles the block touches -- no tracer axis: the value tracers are
//   a loop inside the kernel, so that the condition is read once for all of them.  A lane owns one element and walks its
//   interior column slots (mpdata_wm_walk.h) as linear streams, NB columns in flight: the tc stream at j.prv + tc *
//   prv_tstride, a value tracer at the signed 64-bit offset (t - tc) * prv_tstride from it (t < tc: a negative offset).
//   lo and hi sit in registers, every accumulator is lane-local in column order.  No LDS, no barrier, no cross-lane
//   traffic.  Two forms with the same bits:
//     MASK     nx <= 64 (MASK_NX) and two value tracers or more: one walk over the tc stream forms cnt, the sum of c under its own condition and a
//              64-bit in-mask per lane and half (two 32-bit registers; a batch of NB columns is one byte of it,
//              tested at compile-time positions); then one walk per value tracer adds under the mask.  The walk of t == tc is
//              the first one: its sum is kept, not read again.
//     RE-READ  every other call (nx > 64; cnt alone; one value tracer): per value tracer the tc stream and the t stream are walked together (one stream for t ==
//              tc) and the comparison is made again; cnt comes from the first of these walks (csum NULL: a walk of tc
//              alone).
//   sel: the block (mpdata_wm_walk.h).  A slot that is no instance of it -- padding, the phantom half of an odd fp32 plan,
//     the partner of a split pair, a neighbour in the tile -- reaches no output; a wave none of whose elements is in the
//     block (or owned, W > 1) loads nothing.
//     W > 1 (windowed plans): only the levels a window OWNS are read, each with lo / hi of the tall level it stands for,
//     and each is written to that tall level.  The caller need not refresh the seams in front.
struct MpdataLevelCondJob {
  MpdataLayoutJob j;
  MpdataBlockSel sel;
  int tc;           // the condition tracer
  int first, ntr;   // the value tracers (csum NULL: not looked at)
  const void* lo;   // NULL: no lower bound
  const void* hi;   // NULL: no upper bound (one of the two is given)
  void* cnt;        // NULL: not wanted
  void* csum;       // NULL: not wanted (one of the two is given)
};
hipError_t mpdata_level_cond_wm(const MpdataLevelCondJob& b, hipStream_t stream);

// Reference layout: f(ld, -2:nx+3, nlev, ntr_all) with elem_bytes = 4 or 8, instances [sl0, sl0 + n) of its ld.  One thread
// per instance and level row, loops over i, 64-bit offsets (a value tracer's row at a signed offset from the tc row): the
// re-read walk.
hipError_t mpdata_level_cond_ref(const void* f, int elem_bytes, long long ld, long long sl0, long long n, int nx, int nlev, int ntr_all,
                                 int tc, const void* lo, const void* hi, void* cnt, void* csum, int first, int ntr, hipStream_t stream);

#endif
