// mpdata_scale_uw.h -- host interface of the velocity-scaling kernels (mpdata_scale_uw.hip; include/mpdata_hip.h 3j):
// per instance one factor, multiplied into EVERY column and level of one velocity array (u or w), in place:
//   a(sl, :, :) = a(sl, :, :) * s(sl - sl0)       one rounded multiply in the array's precision, the factor as given
// s is an array of n reals of that precision, the block's first instance at index 0.  It is only read, and nothing
// outside it is.  One call scales one array; u and w are two calls.
#ifndef MPDATA_SCALE_UW_H
#define MPDATA_SCALE_UW_H
#include <hip/hip_runtime.h>

#include "mpdata_wm_walk.h"

// Plan layout.  j: the plan side of the array exactly as wm_job(which = 1 or 2) makes it (strides in 8-byte elements;
// j.ref is not used).  The kernel needs the storage layout only: element e = s * nlev + kk of column slot c of a tile,
// split into whole 128-byte lines and a rest (mpdata_layout.h); it walks the column slots the array stores,
// c = j.prv_col0 .. j.prv_col0 + j.ncols - 1.
//   sel: the block (mpdata_wm_walk.h; the launcher checks sel.nz with the rest, the kernel does not look at it).  A
//     slot that is no instance of the block keeps its bits (the partner half of a split pair is stored back as it was
//     loaded).  The one exception is the PHANTOM of an odd fp32 plan (include/mpdata_hip.h 3f): it takes the factor of the
//     last instance whenever the block holds that instance, and so stays its copy.  Every window of a windowed plan,
//     and every level it stores (owned or not), takes the factor of its instance.
struct MpdataScaleUwJob {
  MpdataLayoutJob j;
  MpdataBlockSel sel;
  const void* s;
};
// the grid covers the tiles the block touches
hipError_t mpdata_scale_uw_wm(const MpdataScaleUwJob& b, hipStream_t stream);

// Reference layout: a(ld, ncols, nlevs) with elem_bytes = 4 or 8 (u: ncols = nx + 5, nlevs = nzm; w: nx + 4, nz),
// instances [sl0, sl0 + n) of its ld; one thread per instance, 64-bit offsets.
hipError_t mpdata_scale_uw_ref(void* a, int elem_bytes, long long ld, long long sl0, long long n, int ncols, int nlevs,
                               const void* s, hipStream_t stream);

#endif
