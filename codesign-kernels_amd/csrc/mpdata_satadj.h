// mpdata_satadj.h -- host interface of the saturation adjustment of a plan's tracers, in place (mpdata_satadj.hip;
// include/mpdata_hip.h 3y): per instance sl of the block (b = sl - sl0), level k = 1 .. nlev and INTERIOR column
// i = 1 .. nx the condensate qn (tracer tn) and, on request, the temperature T (tracer tt) are diagnosed from a conserved
// temperature-like tracer th and total water tq by a Newton iteration on the caller's saturation curves.  Every
// statement is rounded once in the arrays' precision, in this association, no contraction, every divide an IEEE divide,
// comparisons plain compare-and-select (the header has the algorithm line by line; satadj_cells in the .hip follows it).
// pres, gz, ncld, iters (n, nlev): reference layout, leading dimension n, the block's first instance at index 0.  th, tq,
// pres and gz are only read; halo columns and every other tracer are neither read nor written; a row with pres == 0
// keeps every bit of tn and tt and is not stored.
#ifndef MPDATA_SATADJ_H
#define MPDATA_SATADJ_H
#include <hip/hip_runtime.h>

#include "mpdata_wm_walk.h"

// the caller's numbers in the precision of the arrays, each rounded once; an = 1 / (tmax - tmin), bn = tmin * an and
// lf = ls - lv are formed on the host in that precision, each operation rounded once
template <typename R>
struct MpdataSatadjPar {
  R esw[9], desw[9], esi[9], desi[9];
  R t0, xmin, eps, lv, ls, lf, tmin, tmax, an, bn, tol;
  int maxit;
};

// what both layouts take: the four tracers (tt = -1: T is not stored), the rows and the numbers
struct MpdataSatadjArgs {
  int th, tq, tn, tt;
  const void* pres;
  const void* gz;    // NULL: T1 = h
  int ice;           // != 0: the ice curve and the mixed-phase ramp between tmin and tmax
  void* ncld;        // NULL: not wanted
  void* iters;       // NULL: not wanted
  union {
    MpdataSatadjPar<double> d;
    MpdataSatadjPar<float> f;
  } par;             // the member of the arrays' precision is filled
};

// Plan layout.  j: the plan side of f exactly as wm_job(which = 0) makes it for ALL tracers of the plan (j.prv on tracer
// 0, strides in 8-byte elements; j.ref is not used); the four tracers distinct, in [0, j.ntr).
//   The grid runs over (tile, 64-element slice) of the tiles the block touches -- no tracer axis.  A lane owns one
//   element and walks its interior column slots (mpdata_wm_walk.h) as streams at signed 64-bit offsets from tracer th:
//   two read streams (th, tq), one or two write streams (tn, tt), MPDATA_SATADJ_NC columns of a lane at a time, the next
//   batch's loads in flight while this batch iterates.  p, 1 / p and gz of the lane's instance and level are in registers
//   per half.  The Newton loops of the batch's cells run interleaved under one joint exit, predicated per cell: a
//   finished cell keeps its T, qs, dq and d by select; the loop ends for the wave when a __ballot finds no cell active.
//   No LDS, no barrier, no other cross-lane traffic.
//   sel: the block (mpdata_wm_walk.h).  A slot that is no instance of it, or whose pres is 0, keeps its bits (the partner
//     half of such a pair is loaded from tn and tt and stored back as loaded -- the only reads of tn and tt; a lane none
//     of whose halves is on stores nothing).  The PHANTOM of an odd fp32 plan takes the result of the plan's last slot in
//     tn and tt whenever the block holds that instance and its pres is not zero on that level (W > 1: the kernel leaves
//     the inner plan's phantom alone and the caller restores it behind the call).
//     W > 1 (windowed plans): only the levels a window OWNS are read and written, each with pres and gz of the tall level
//     it stands for; ncld and iters are written by each level's owner.  No seam refresh in front; the caller marks the
//     seams of tn and tt stale afterwards.
#ifndef MPDATA_SATADJ_NC
#define MPDATA_SATADJ_NC 2   // columns of a lane whose Newton loops are interleaved (docs/EXPERIMENTS.md AI: 1, 2, 4, 8 timed)
#endif
struct MpdataSatadjJob {
  MpdataLayoutJob j;
  MpdataBlockSel sel;
  MpdataSatadjArgs a;
};
hipError_t mpdata_satadj_wm(const MpdataSatadjJob& b, hipStream_t stream);

// Reference layout: f(ld, -2:nx+3, nlev, ntr) with elem_bytes = 4 or 8, instances [sl0, sl0 + n) of its ld.  One thread
// per instance and level row, one loop over i, 64-bit offsets (the rows of tq, tn, tt at signed offsets from the row of
// th): a thread reads its own row of th and tq and writes its own row of tn and tt only.
hipError_t mpdata_satadj_ref(void* f, int elem_bytes, long long ld, long long sl0, long long n, int nx, int nlev, int ntr,
                             const MpdataSatadjArgs& a, hipStream_t stream);

#endif
