// mpdata_subside.h -- host interface of the large-scale vertical advection of f, in place (mpdata_subside.hip;
// include/mpdata_hip.h 3m): per instance sl of the block, tracer t, level k = 1 .. nlev, kb = max(1, k-1), kc = min(nlev, k+1)
// and EVERY column slot i = -2 .. nx+3, every f on the right the value BEFORE the call, every operation rounded once in
// the arrays' precision, in this association, no contraction:
//   dec(i,k) = cb(sl,k) * (f(i,k) - f(i,kb)) + cc(sl,k) * (f(i,kc) - f(i,k))
//   f(i,k)   = f(i,k) - dec(i,k)
//   dsum(sl,k,t) : s = +0; do i = 1, nx: s = s + dec(i,k)                               (NULL: skipped)
// cb, cc (n, nlev), dsum (n, nlev, ntr): reference layout, leading dimension n, the block's first instance at index 0.
// cb and cc are only read, and nothing outside them is; at a clamped level the neighbour IS the level itself, so the
// difference is an exact zero whatever the coefficient.
#ifndef MPDATA_SUBSIDE_H
#define MPDATA_SUBSIDE_H
#include <hip/hip_runtime.h>

#include "mpdata_wm_walk.h"

// Plan layout.  j: the plan side of f exactly as wm_job(which = 0) makes it for tracers [first, first + j.ntr) (j.prv on
// the first of them, strides in 8-byte elements; j.ref is not used).
//   sel: the block (mpdata_wm_walk.h).  A slot that is no instance of it keeps its bits (the partner half of a split
//     pair is stored back as it was loaded).  The PHANTOM of an odd fp32 plan takes the result of the plan's last slot,
//     its partner in the pair, whenever the block holds that instance: it was that slot's copy on every column before
//     the call, so this is what the same operations on the same inputs give.
//     W > 1 (windowed plans): only the levels a window OWNS are written, each with the coefficients of the tall level it
//     stands for, and dsum is written by the owner -- every tall level once.  An owned level lies 3 or more levels
//     inside the artificial edges of its window, so its two neighbours are levels the window stores; the caller has
//     refreshed the seams, and marks them stale afterwards.
struct MpdataSubsideJob {
  MpdataLayoutJob j;
  MpdataBlockSel sel;
  const void *cb, *cc;
  void* dsum;
};
// the grid covers the tiles the block touches; a workgroup owns whole tiles
hipError_t mpdata_subside_wm(const MpdataSubsideJob& b, hipStream_t stream);

// Reference layout: f(ld, -2:nx+3, nlev, ntr) with elem_bytes = 4 or 8, instances [sl0, sl0 + n) of its ld.  One thread
// per instance and (level, tracer) row, 64-bit offsets.  Out of place and back: `scratch` (n * (nx + 6) * nlev * ntr
// reals, device memory of the caller's) takes the new rows, a second kernel on the same stream copies them into f --
// rows k +- 1 belong to threads of other workgroups, and nothing but the kernel boundary orders those.
hipError_t mpdata_subside_ref(void* f, int elem_bytes, long long ld, long long sl0, long long n, int nx, int nlev, int ntr,
                              const void* cb, const void* cc, void* dsum, void* scratch, hipStream_t stream);

#endif
