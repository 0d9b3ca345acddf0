// mpdata_diffuse.h -- host interface of the eddy diffusion of f, in place (mpdata_diffuse.hip; include/mpdata_hip.h 3l):
// per instance sl of the block, tracer t, level k = 1 .. nzm and interior column i = 1 .. nx, every f on the right the
// value BEFORE the call, every operation rounded once in the arrays' precision, in this association, no contraction:
//   Fx(i,k) = -((cx(sl,k) * (tkh(sl,i,k) + tkh(sl,i+1,k))) * (f(i+1,k) - f(i,k)))      i = 0 .. nx
//   Fz(i,k) = -((cz(sl,k) * (tkh(sl,i,k) + tkh(sl,i,k+1))) * (f(i,k+1) - f(i,k)))      k = 1 .. nzm - 1
//   Fz(i,0) = sb(sl,i) (+0: NULL), Fz(i,nzm) = st(sl,i) (+0: NULL),  ir(k) = 1 / (rho(sl,k) * adz(sl,k))
//   f(i,k)  = f(i,k) - ((Fx(i,k) - Fx(i-1,k)) + (Fz(i,k) - Fz(i,k-1)) * ir(k))
//   zflux(sl,k',t) : s = +0; do i = 1, nx: s = s + Fz(i,k'-1)                          k' = 1 .. nz (NULL: skipped)
// cx, cz (n, nlev), sb, st (n, nx), zflux (n, nlev + 1, ntr): reference layout, leading dimension n, the block's first
// instance at index 0.  cz(:, nlev) is never read.  Only the interior columns of f are written; columns 0 and nx+1 are read.
#ifndef MPDATA_DIFFUSE_H
#define MPDATA_DIFFUSE_H
#include <hip/hip_runtime.h>

#include "mpdata_wm_walk.h"

// Plan layout.  j: the plan side of f exactly as wm_job(which = 0) makes it for tracers [first, first + j.ntr) (j.prv on
// the first of them; strides in 8-byte elements; j.ref is not used).
//   tkh: the diffusivity IN THE PLAN LAYOUT -- one array shaped as one tracer of f (the same tile stride, chunk and
//     main / rest split), column i = 0 .. nx+1 at column slot i + 2; only the slots of the block's instances need hold
//     anything (the other halves are computed on whatever is there and thrown away).
//   rho, adz: the plan's unsplit [tile][3][instance][level] array, element e of tile t at base + t * kc_tile_stride + e.
//   sel: the block (mpdata_wm_walk.h; W = 1: windowed plans are not supported).  A slot that is no instance of it keeps
//     its bits (the partner half of a split pair is stored back as it was loaded).  The PHANTOM of an odd fp32 plan takes
//     the result of instance ncrms - 1, its partner in the pair, whenever the block holds that instance: it was that
//     instance's copy on every column before the call, so this is what the same operations on the same inputs give.
struct MpdataDiffuseJob {
  MpdataLayoutJob j;
  MpdataBlockSel sel;
  const void* tkh;
  const void *rho, *adz;
  long long kc_tile_stride;
  const void *cx, *cz, *sb, *st;
  void* zflux;
};
// the grid covers the tiles the block touches; a workgroup owns whole tiles
hipError_t mpdata_diffuse_wm(const MpdataDiffuseJob& b, hipStream_t stream);

// Reference layout: f(ld, -2:nx+3, nlev, ntr), rho(ld, nlev), adz(ld, nlev) with elem_bytes = 4 or 8, instances
// [sl0, sl0 + n) of their ld; tkh (n, 0:nx+1, nlev) and the other arrays as above.  One thread per instance, 64-bit
// offsets.  Out of place and back: `scratch` (n * nx * nlev * ntr reals, device memory of the caller's) takes the new
// interior, a second kernel on the same stream copies it into f -- rows of different levels depend on each other, and
// nothing but the kernel boundary orders threads of different workgroups.
hipError_t mpdata_diffuse_ref(void* f, const void* rho, const void* adz, int elem_bytes, long long ld, long long sl0, long long n,
                              int nx, int nlev, int ntr, const void* tkh, const void* cx, const void* cz, const void* sb,
                              const void* st, void* zflux, void* scratch, hipStream_t stream);

#endif
