// mpdata_vsolve.h -- host interface of the implicit vertical solve of f, in place (mpdata_vsolve.hip; include/mpdata_hip.h
// 3o): per instance sl of the block, tracer t and INTERIOR column i = 1 .. nx the tridiagonal system
//   lo(k) x(k-1) + di(k) x(k) + up(k) x(k+1) = f(i,k)          k = 1 .. nlev
// solved without pivoting, every statement one rounded operation in the arrays' precision, nothing contracted, the
// divide IEEE:
//   factors, per (sl,k):   p(1) = 1 / di(1);  g(1) = up(1) * p(1)
//                          k = 2 .. nlev:  m = lo(k) * g(k-1);  d = di(k) - m;  p(k) = 1 / d;  g(k) = up(k) * p(k)
//   per (sl,i,t):          y(1) = f(i,1) * p(1);   k = 2 .. nlev:  m = lo(k) * y(k-1);  r = f(i,k) - m;  y(k) = r * p(k)
//                          x(nlev) = y(nlev);      k = nlev-1 .. 1:  m = g(k) * x(k+1);  x(k) = y(k) - m;   f(i,k) = x(k)
// lo, di, up, p, g (n, nlev): reference layout, leading dimension n, the block's first instance at index 0; lo(:,1) and
// up(:,nlev) are never read.  Halo columns of f are neither read nor written.
//   The sweeps run y(1) and x(nlev) through the general statement with a carried +0 and a staged +0 coefficient:
//   +0 * +0 = +0 and v - (+0) = v for every v, -0.0 included, so the bits are those of the definition.
#ifndef MPDATA_VSOLVE_H
#define MPDATA_VSOLVE_H
#include <hip/hip_runtime.h>

#include "mpdata_wm_walk.h"

// The factors p and g (n * nlev reals each, device memory of the caller's) from lo, di, up: one thread per instance,
// sequential in k, coalesced along sl.  g(:,nlev) is written as +0.
hipError_t mpdata_vsolve_factor(const void* lo, const void* di, const void* up, int elem_bytes, long long n, int nlev, void* p, void* g,
                                hipStream_t stream);

// Plan layout.  j: the plan side of f exactly as wm_job(which = 0) makes it for tracers [first, first + j.ntr) (j.prv on
// the first of them, strides in 8-byte elements; j.ref is not used); lo: the caller's; pg: p and, behind its n * nlev
// reals, g, from mpdata_vsolve_factor (nlev of the TALL column).
//   sel: the block (mpdata_wm_walk.h).  A slot that is no instance of it keeps its bits (the partner half of a split
//     pair is stored back as it was loaded).  The PHANTOM of an odd fp32 plan takes the result of the plan's last slot,
//     its partner in the pair, whenever the block holds that instance.
//     W > 1 (windowed plans): only the levels a window OWNS are read and written, each with the coefficients of the tall
//     level it stands for.  The forward sweep walks the windows upward and stores y, the backward sweep walks them
//     downward and stores x: f is read twice and written twice.  The phantom keeps its bits: the caller restores it.
struct MpdataVsolveJob {
  MpdataLayoutJob j;
  MpdataBlockSel sel;
  const void *lo, *pg;
};
hipError_t mpdata_vsolve_wm(const MpdataVsolveJob& b, hipStream_t stream);

// Reference layout: f(ld, -2:nx+3, nlev, ntr) with elem_bytes = 4 or 8, instances [sl0, sl0 + n) of its ld.  One thread per
// instance, grid.y over the (column, tracer) rows, 64-bit offsets.  A thread owns its column: y and then x go into f in
// place.
hipError_t mpdata_vsolve_ref(void* f, int elem_bytes, long long ld, long long sl0, long long n, int nx, int nlev, int ntr, const void* lo,
                             const void* p, const void* g, hipStream_t stream);

#endif
