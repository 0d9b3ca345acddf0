// mpdata_column_path.h -- host interface of the mass-weighted column integrals (mpdata_column_path.hip;
// include/mpdata_hip.h 3k): per instance sl, interior column i = 1 .. nx and tracer t
//   wgt(sl,k)    = rho(sl,k) * adz(sl,k)
//   path(sl,i,t) : s = +0.0; do k = 1, nzm:  s = s + wgt(sl,k) * f(sl,i,k,t)
//   mass(sl,t)   : s = +0.0; do i = 1, nx:   s = s + path(sl,i,t)
// every operation rounded once in the arrays' precision, in this order and association, no contraction.
//   path: reference layout (n, nx, ntr), leading dimension n, the block's first instance at index 0, tracer slowest;
//   mass: (n, ntr), formed from path by a second kernel on the same stream; NULL: skipped.
// Halo columns of f are never read.
#ifndef MPDATA_COLUMN_PATH_H
#define MPDATA_COLUMN_PATH_H
#include <hip/hip_runtime.h>

#include "mpdata_wm_walk.h"

// Plan layout.  j: the plan side of f exactly as wm_job(which = 0) makes it for tracers [first, first + j.ntr) (j.prv on
// the first of them; strides in 8-byte elements; j.ref is not used); rho, adz: that array's slab in the plan's unsplit
// [tile][3][instance][level] array, element e of tile t at base + t * kc_tile_stride + e.
//   sel: the block (mpdata_wm_walk.h).  Of a windowed plan only the OWNED levels of every window are read, each window's
//   with its own weights, in rising order of the tall level.
struct MpdataColumnPathJob {
  MpdataLayoutJob j;
  const void *rho, *adz;
  long long kc_tile_stride;
  MpdataBlockSel sel;
  void *path, *mass;
};
// the grid covers the tiles the block touches
hipError_t mpdata_column_path_wm(const MpdataColumnPathJob& b, hipStream_t stream);

// Reference layout: f(ld, -2:nx+3, nlev, ntr), rho(ld, nlev), adz(ld, nlev) with elem_bytes = 4 or 8, instances
// [sl0, sl0 + n) of their ld; one thread per instance, 64-bit offsets.
hipError_t mpdata_column_path_ref(const void* f, const void* rho, const void* adz, int elem_bytes, long long ld, long long sl0,
                                  long long n, int nx, int nlev, int ntr, void* path, void* mass, hipStream_t stream);

#endif
