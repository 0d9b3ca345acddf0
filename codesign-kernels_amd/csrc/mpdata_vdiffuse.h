// mpdata_vdiffuse.h -- host interface of the implicit vertical diffusion of f with a per-cell diffusivity, in place
// (mpdata_vdiffuse.hip; include/mpdata_hip.h 3s): per instance sl of the block, tracer t and INTERIOR column i = 1 .. nx
// backward Euler of 3l's vertical part, the tridiagonal matrix of the column formed from tkh and cz and solved without
// pivoting, every statement one rounded operation in the arrays' precision, nothing contracted, the divides IEEE:
//   ir(k)  = 1 / (rho(k) * adz(k))
//   e(k)   = cz(k) * (tkh(i,k) + tkh(i,k+1))   k = 1 .. nlev-1;   e(0) = e(nlev) = +0
//   a(k)   = e(k-1) * ir(k);  c(k) = e(k) * ir(k);  t = 1 + a(k);  di(k) = t + c(k)
//   r(k)   = f(i,k),  r(1) = f(i,1) + sb(i) * ir(1),  r(nlev) = f(i,nlev) - st(i) * ir(nlev)      (NULL sb / st: skipped)
//   forward:   p = 1 / di(1);  g(1) = c(1) * p;  y(1) = r(1) * p
//              k = 2 .. nlev:  m = a(k) * g(k-1);  d = di(k) - m;  p = 1 / d;  g(k) = c(k) * p
//                              q = a(k) * y(k-1);  v = r(k) + q;   y(k) = v * p
//   backward:  x(nlev) = y(nlev);  k = nlev-1 .. 1:  m = g(k) * x(k+1);  x(k) = y(k) + m;   f(i,k) = x(k)
// tkh (n, 0:nx+1, nlev), cz (n, nlev), sb, st (n, nx): reference layout, leading dimension n, the block's first instance
// at index 0; tkh's columns 0 and nx+1 and cz(:,nlev) are never read.  Halo columns of f are neither read nor written.
//   Level 1 and level nlev are NOT run through the general statements with a carried +0, as mpdata_vsolve.h does: here the
//   general statements ADD (v = r + q, x = y + m), and -0.0 + +0 is +0.0 where the definition keeps -0.0.
#ifndef MPDATA_VDIFFUSE_H
#define MPDATA_VDIFFUSE_H
#include <hip/hip_runtime.h>

#include "mpdata_wm_walk.h"

// Plan layout, plain plans only (sel.W == 1).  j: the plan side of f exactly as wm_job(which = 0) makes it for tracers
// [first, first + j.ntr); rho, adz, kc_tile_stride: the plan's kc array as mpdata_sediment.h takes it.
//   ir: device memory of n * nlev reals of the caller's; a small kernel in front of the sweeps writes 1 / (rho * adz) there.
//   sel: the block.  A slot that is no instance of it keeps its bits (the partner half of a split pair is stored back as
//   it was loaded); the PHANTOM of an odd fp32 plan takes the result of the plan's last slot whenever the block holds
//   that instance.
struct MpdataVdiffuseJob {
  MpdataLayoutJob j;
  MpdataBlockSel sel;
  const void *rho, *adz;
  long long kc_tile_stride;
  void* ir;
  const void *tkh, *cz, *sb, *st;   // sb, st: may be NULL
};
hipError_t mpdata_vdiffuse_wm(const MpdataVdiffuseJob& b, hipStream_t stream);

// Reference layout: f(ld, -2:nx+3, nlev, ntr), rho, adz (ld, nlev) with elem_bytes = 4 or 8, instances [sl0, sl0 + n) of
// their ld.  One thread per instance and column, grid.y over the columns, the tracers one after the other inside the
// thread; 64-bit offsets.  A thread owns its columns: y and then x go into f in place, g(k) into gbuf (n * nx * nlev reals
// of the caller's, element (b, i, k) at b + n * ((i - 1) + nx * (k - 1))), written and read back by the same thread.
hipError_t mpdata_vdiffuse_ref(void* f, const void* rho, const void* adz, int elem_bytes, long long ld, long long sl0, long long n,
                               int nx, int nlev, int ntr, const void* tkh, const void* cz, const void* sb, const void* st, void* gbuf,
                               hipStream_t stream);

#endif
