// mpdata_column_step.h -- host interface of the fused column step of f, in place (mpdata_column_step.hip;
// include/mpdata_hip.h 3q): per instance sl of the block, tracer t and INTERIOR column i = 1 .. nx up to four stages in this
// fixed order, each reading the field the stage before left, every f on the right of a stage the value BEFORE that stage,
// every operation rounded once in the arrays' precision, in the association of the single calls, nothing contracted, the
// divides IEEE:
//   1 source    (s)            p = c * s(sl,i,k,t);  g = f(i,k) + p;  clip: g = max(0, g)                        (3p)
//   2 subside   (cb, cc)       kb = max(1,k-1), kc = min(nlev,k+1):
//                              f(i,k) = f(i,k) - (cb(k) * (f(i,k) - f(i,kb)) + cc(k) * (f(i,kc) - f(i,k)))      (3m)
//   3 sediment  (wp)           Fz(k) = wp(sl,i,k,t) * f(i,k), Fz(nlev+1) = +0;  ir(k) = 1 / (rho(k) * adz(k));
//                              f(i,k) = f(i,k) - (Fz(k) - Fz(k+1)) * ir(k);  psfc(sl,i,t) = Fz(1)               (3n)
//   4 vsolve    (lo, p, g)     y(k) = (f(i,k) - lo(k) * y(k-1)) * p(k) upward, x(k) = y(k) - g(k) * x(k+1) downward  (3o)
// A stage whose arrays are NULL is absent.  s, wp (n, nx, nlev, ntr), psfc (n, nx, ntr), cb, cc, lo, p, g (n, nlev):
// reference layout, leading dimension n, the block's first instance at index 0; p and g from mpdata_vsolve_factor.  Halo
// columns are neither read nor written; no horizontal sum is formed.
//   One lane owns one column and sweeps it in place.  Stages 1 - 3 and the forward sweep of stage 4 share ONE upward pass:
//   the source is applied as a level is read, the level below and the level itself after stage 1 are carried in registers
//   and level k + 1 is read before level k is written (stage 2); stage 3 finishes level k - 1 once Fz(k) is known, from
//   the carried f(k-1) and Fz(k-1) after stage 2; the forward sweep consumes each finished level.  Every operation has the
//   operands it has in the single calls, hence their bits.  A second, downward pass is the backward sweep.
#ifndef MPDATA_COLUMN_STEP_H
#define MPDATA_COLUMN_STEP_H
#include <hip/hip_runtime.h>

#include "mpdata_wm_walk.h"

// what the sweeps read besides f: NULL = the stage is absent (cb with cc, lo with pg)
struct MpdataColumnStepArrays {
  const void *s, *cb, *cc, *wp, *lo, *pg;   // pg: p, and g behind its n * nlev reals
  void* psfc;                               // may be NULL; only with wp
  double c;                                 // rounded once to the arrays' precision
  int clip;
};

// Plan layout, plain plans only (sel.W == 1).  j: the plan side of f exactly as wm_job(which = 0) makes it for tracers
// [first, first + j.ntr); rho, adz, kc_tile_stride: the plan's kc array as mpdata_sediment.h takes it (read with wp only).
//   The geometry and the copy stage of mpdata_vsolve.hip: a workgroup takes UG adjacent units and CB columns, its four
//   waves copy the column slots as linear streams into LDS [column][unit][level] (odd level stride), a lane per (unit,
//   column) sweeps, the waves copy back.  s, wp and the coefficient rows are read by the sweeping lanes from the caller's
//   arrays, the unit fastest; so is ir = 1 / (rho * adz) (n, nlev), which a small kernel in front forms from the plan's
//   kc array into the job's `ir`, as mpdata_vsolve_factor forms p and g.
//   sel: the block.  A slot that is no instance of it keeps its bits; the PHANTOM of an odd fp32 plan takes the result of
//   the plan's last slot whenever the block holds that instance.
struct MpdataColumnStepJob {
  MpdataLayoutJob j;
  MpdataBlockSel sel;
  const void *rho, *adz;
  long long kc_tile_stride;
  void* ir;   // with wp: device memory of n * nlev reals of the caller's, written by a small kernel in front of the sweeps
  MpdataColumnStepArrays a;
};
hipError_t mpdata_column_step_wm(const MpdataColumnStepJob& b, hipStream_t stream);

// Reference layout: f(ld, -2:nx+3, nlev, ntr), rho, adz (ld, nlev; read with wp only) with elem_bytes = 4 or 8, instances
// [sl0, sl0 + n) of their ld.  One thread per instance, grid.y over the (column, tracer) rows, 64-bit offsets.  A thread
// owns its column: in place, no scratch array.
hipError_t mpdata_column_step_ref(void* f, const void* rho, const void* adz, int elem_bytes, long long ld, long long sl0, long long n,
                                  int nx, int nlev, int ntr, const MpdataColumnStepArrays& a, hipStream_t stream);

#endif
