// mpdata_courant.h -- host interface of the outflow-Courant-number kernels (mpdata_courant.hip; include/mpdata_hip.h 3h):
// per instance sl, interior column i = 1 .. nx and level k = 1 .. nzm
//   a = max(0, u(sl,i+1,k)) - min(0, u(sl,i,k))
//   b = max(0, wk1) - min(0, w(sl,i,k))            wk1 = w(sl,i,k+1), and +0 at k = nzm (the routine's www(nz) = 0)
//   c = (a + b * iadz) * irho                      iadz = 1 / adz(sl,k), irho = 1 / rho(sl,k)
// every operation rounded once in the arrays' precision, no contraction, IEEE divides; the sign of c is cleared.
//   clev(sl,k) = max of c over i (reference layout (n, nzm), leading dimension n, the block's first instance at index 0),
//   cinst(sl)  = max of clev(sl,k) over k (n reals).  Either may be NULL, not both.
// cinst is formed by an unsigned integer atomic max on the bit pattern (c >= +0: the unsigned order of the bits is the
// numeric order), so the calls zero it first, on the same stream.  Velocity halos are never read.
#ifndef MPDATA_COURANT_H
#define MPDATA_COURANT_H
#include <hip/hip_runtime.h>

#include "mpdata_wm_walk.h"

// Plan layout.  j: the plan side of u exactly as wm_job(which = 1) makes it (strides in 8-byte elements, j.prv_col0 = 1;
// j.ref is not used); w: the plan side of w (the same geometry, another base); rho, adz: that array's slab in the plan's
// unsplit [tile][3][instance][level] array, element e of tile t at base + t * kc_tile_stride + e.
//   sel: the block (mpdata_wm_walk.h).  Only OWNED levels of a windowed plan reach the outputs (an owned level's k + 1
//   lies inside its window; the last window's top is the real level nz, the +0).
struct MpdataCourantJob {
  MpdataLayoutJob j;
  const void *w, *rho, *adz;
  long long kc_tile_stride;
  MpdataBlockSel sel;
  void *clev, *cinst;
};
// the grid covers the tiles the block touches; cinst (if given) is zeroed first
hipError_t mpdata_courant_wm(const MpdataCourantJob& b, hipStream_t stream);

// Reference layout: u(ld, -1:nx+3, nzm), w(ld, -1:nx+2, nz), rho(ld, nzm), adz(ld, nzm) with elem_bytes = 4 or 8,
// instances [sl0, sl0 + n) of their ld; one thread per instance, 64-bit offsets; cinst (if given) is zeroed first.
hipError_t mpdata_courant_ref(const void* u, const void* w, const void* rho, const void* adz, int elem_bytes, long long ld,
                              long long sl0, long long n, int nx, int nz, void* clev, void* cinst, hipStream_t stream);

#endif
