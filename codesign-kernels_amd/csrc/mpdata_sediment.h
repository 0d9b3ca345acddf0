// mpdata_sediment.h -- host interface of the sedimentation of f, in place (mpdata_sediment.hip; include/mpdata_hip.h
// 3n): per instance sl of the block, tracer t, INTERIOR column i = 1 .. nx and level k = 1 .. nlev, every f on the right
// the value BEFORE the call, every operation rounded once in the arrays' precision, in this association, no contraction,
// the divide IEEE:
//   Fz(i,k)      = wp(sl,i,k,t) * f(i,k)          k = 1 .. nlev;   Fz(i,nlev+1) = +0
//   ir(k)        = 1 / (rho(sl,k) * adz(sl,k))
//   f(i,k)       = f(i,k) - (Fz(i,k) - Fz(i,k+1)) * ir(k)
//   psfc(sl,i,t)  = Fz(i,1)                                                             (NULL: skipped)
//   pflux(sl,k,t) : s = +0; do i = 1, nx: s = s + Fz(i,k)                               (NULL: skipped)
// wp (n, nx, nlev, ntr), psfc (n, nx, ntr), pflux (n, nlev, ntr): reference layout, leading dimension n, the block's first
// instance at index 0.  wp is only read, and nothing outside it is; halo columns are neither read nor written.
#ifndef MPDATA_SEDIMENT_H
#define MPDATA_SEDIMENT_H
#include <hip/hip_runtime.h>

#include "mpdata_wm_walk.h"

// Plan layout.  j: the plan side of f exactly as wm_job(which = 0) makes it for tracers [first, first + j.ntr) (j.prv on
// the first of them, strides in 8-byte elements; j.ref is not used); rho, adz, kc_tile_stride: the plan's kc array as the
// column integrals take it (mpdata_column_path.h).
//   wp is read where it lies: a workgroup owns the whole tiles of a group of adjacent 8-byte elements of the instance
//     axis (16: a row of wp of the group is 128 bytes of fp64, 256 of fp32; fewer where the levels would not fit) and
//     copies the group's rows of a column batch into LDS as [column][unit][level].  Nothing of wp goes to device memory.
//   sel: the block (mpdata_wm_walk.h).  A slot that is no instance of it keeps its bits (the partner half of a split
//     pair is stored back as it was loaded).  The PHANTOM of an odd fp32 plan takes the result of the plan's last slot,
//     its partner in the pair, whenever the block holds that instance.
//     W > 1 (windowed plans): only the levels a window OWNS are written, each with wp and ir of the tall level it
//     stands for; psfc is Fz of tall level 1 (level 1 of window 0), pflux is written by each level's owner.  An owned level lies 3 or
//     more levels inside the artificial edges of its window, so level k + 1 is a level the window stores; the caller has
//     refreshed the seams, and marks them stale afterwards.
struct MpdataSedimentJob {
  MpdataLayoutJob j;
  MpdataBlockSel sel;
  const void *rho, *adz;      // the plan's kc array: element e of tile t at rho + t * kc_tile_stride + e
  long long kc_tile_stride;
  const void* wp;
  void *psfc, *pflux;
};
hipError_t mpdata_sediment_wm(const MpdataSedimentJob& b, hipStream_t stream);

// Reference layout: f(ld, -2:nx+3, nlev, ntr), rho, adz (ld, nlev) with elem_bytes = 4 or 8, instances [sl0, sl0 + n) of
// their ld.  One thread per instance and (level, tracer) row, 64-bit offsets.  Out of place and back: `scratch`
// (n * nx * nlev * ntr reals, device memory of the caller's) takes the new interior rows, a second kernel on the same
// stream copies them into f -- row k + 1 belongs to a thread of another workgroup, and nothing but the kernel boundary
// orders those.
hipError_t mpdata_sediment_ref(void* f, const void* rho, const void* adz, int elem_bytes, long long ld, long long sl0, long long n,
                               int nx, int nlev, int ntr, const void* wp, void* psfc, void* pflux, void* scratch, hipStream_t stream);

#endif
