// mpdata_relax.h -- host interface of the relaxation of f to a level profile, in place (mpdata_relax.hip;
// include/mpdata_hip.h 3r): per instance sl of the block (b = sl - sl0), tracer t, level k = 1 .. nlev and INTERIOR column
// i = 1 .. nx, every operation rounded once in the arrays' precision, in this association, no contraction:
//   target == NULL:  s = +0; do i = 1, nx: s = s + f_old(i,k);   m = s / nx      (nx converted exactly, one IEEE divide)
//   target != NULL:  m = target(b,k,t)
//   mean(b,k,t)   =  m                                                           (NULL: skipped)
//   c(b,k) == 0   :  the level keeps every bit and is not stored
//   else per i    :  d = f_old(i,k) - m;   p = c(b,k) * d;   f(i,k) = f_old(i,k) - p
// c (n, nlev), target and mean (n, nlev, ntr): reference layout, leading dimension n, the block's first instance at index
// 0.  c and target are only read, and nothing outside the arrays is touched; halo columns are neither read nor written.
#ifndef MPDATA_RELAX_H
#define MPDATA_RELAX_H
#include <hip/hip_runtime.h>

#include "mpdata_wm_walk.h"

// Plan layout.  j: the plan side of f exactly as wm_job(which = 0) makes it for tracers [first, first + j.ntr) (j.prv on
// the first of them, strides in 8-byte elements; j.ref is not used).
//   A lane owns one element and walks its interior column slots (mpdata_wm_walk.h): with a target one walk that loads and
//   stores f; without one, for nx <= 32 the KEPT form -- the nx columns of the element are loaded into registers once,
//   summed, updated and stored -- and above it the RE-READ form: the summing walk of mpdata_stats.hip, the divide, and
//   the updating walk over the columns the lane has just read.  No LDS, no barrier: a lane touches the columns of its
//   own element only.
//   sel: the block (mpdata_wm_walk.h).  A slot that is no instance of it keeps its bits (the partner half of a split
//     pair is stored back as it was loaded).  The PHANTOM of an odd fp32 plan takes the result of the plan's last slot,
//     its partner in the pair, whenever the block holds that instance and its c is not zero (W > 1: the kernel leaves the
//     inner plan's phantom alone and the caller restores it behind the call).
//     W > 1 (windowed plans): only the levels a window OWNS are read and written, each with c and the target of the tall
//     level it stands for; mean is written by each level's owner.  The caller need not refresh the seams in front, and
//     marks them stale afterwards.
struct MpdataRelaxJob {
  MpdataLayoutJob j;
  MpdataBlockSel sel;
  const void* c;
  const void* target;   // NULL: relax to the horizontal mean
  void* mean;           // NULL: not wanted
};
hipError_t mpdata_relax_wm(const MpdataRelaxJob& b, hipStream_t stream);

// Reference layout: f(ld, -2:nx+3, nlev, ntr) with elem_bytes = 4 or 8, instances [sl0, sl0 + n) of its ld.  One thread
// per instance and (level, tracer) row, two loops over i, 64-bit offsets, in place: a thread reads and writes its own row
// only.
hipError_t mpdata_relax_ref(void* f, int elem_bytes, long long ld, long long sl0, long long n, int nx, int nlev, int ntr,
                            const void* c, const void* target, void* mean, hipStream_t stream);

#endif
