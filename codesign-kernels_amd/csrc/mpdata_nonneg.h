// mpdata_nonneg.h -- host interface of the conservative per-level non-negativity fixer of f, in place (mpdata_nonneg.hip;
// include/mpdata_hip.h 3x): per instance sl of the block (b = sl - sl0), tracer t, level k = 1 .. nlev and INTERIOR column
// i = 1 .. nx, every operation rounded once in the arrays' precision, in this association, no contraction:
//   s = +0; p = +0; c = +0
//   do i = 1, nx:  x = f_old(i,k);  s = s + x;  y = (x > 0) ? x : +0;  p = p + y;  c = c + ((x < 0) ? 1 : 0)
//   sum(b,k,t) = s;  nneg(b,k,t) = c                                             (NULL: skipped)
//   c == 0      :  the level keeps every bit and is not stored (a -0.0 there stays)
//   c > 0, s > 0:  r = s / p (one IEEE divide);  f(i,k) = y_i * r
//   c > 0, else :  f(i,k) = +0 for every i
// sum and nneg (n, nlev, ntr): reference layout, leading dimension n, the block's first instance at index 0; only written,
// and nothing outside the arrays is touched; halo columns are neither read nor written.
#ifndef MPDATA_NONNEG_H
#define MPDATA_NONNEG_H
#include <hip/hip_runtime.h>

#include "mpdata_wm_walk.h"

// Plan layout.  j: the plan side of f exactly as wm_job(which = 0) makes it for tracers [first, first + j.ntr) (j.prv on
// the first of them, strides in 8-byte elements; j.ref is not used).
//   A lane owns one element and walks its interior column slots (mpdata_wm_walk.h).  nx <= 32, the KEPT form: the nx
//   columns of the element are loaded into registers once, s, p and c are formed, and a lane with c > 0 scales and stores
//   them.  Above it the RE-READ form: a reducing walk, the outputs, and -- unless no lane of the wave has a row in need
//   -- the updating walk over the columns the lane has just read.  A row without a negative cell costs its read and no
//   store in both forms.  No LDS, no barrier: a lane touches the columns of its own element only.
//   sel: the block (mpdata_wm_walk.h).  A slot that is no instance of it keeps its bits (the partner half of a split
//     pair is stored back as it was loaded, as is a half whose row has c == 0 beside one in need).  The PHANTOM of an odd
//     fp32 plan takes the result of the plan's last slot, its partner in the pair, whenever the block holds that instance
//     and its row is rewritten (W > 1: the kernel leaves the inner plan's phantom alone and the caller restores it behind
//     the call).
//     W > 1 (windowed plans): only the levels a window OWNS are read and written; sum and nneg are written by each level's
//     owner at the tall level it stands for.  The caller need not refresh the seams in front, and marks them stale
//     afterwards.
struct MpdataNonnegJob {
  MpdataLayoutJob j;
  MpdataBlockSel sel;
  void* sum;    // NULL: not wanted
  void* nneg;   // NULL: not wanted
};
hipError_t mpdata_nonneg_wm(const MpdataNonnegJob& b, hipStream_t stream);

// Reference layout: f(ld, -2:nx+3, nlev, ntr) with elem_bytes = 4 or 8, instances [sl0, sl0 + n) of its ld.  One thread
// per instance and (level, tracer) row, two loops over i, 64-bit offsets, in place: a thread reads and writes its own row
// only.
hipError_t mpdata_nonneg_ref(void* f, int elem_bytes, long long ld, long long sl0, long long n, int nx, int nlev, int ntr, void* sum,
                             void* nneg, hipStream_t stream);

#endif
