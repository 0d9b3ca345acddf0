// mpdata_level_add.h -- host interface of the level-increment kernels (mpdata_level_add.hip; include/mpdata_hip.h 3i):
// per tracer, instance and level one increment d(sl, k, t), added to EVERY column of f (halo columns included), in place.
//   clip == 0:  f = f + d            one rounded add in the precision of f, the IEEE sign of a zero sum
//   clip != 0:  f = max(0, f + d)    the hardware max on the rounded sum (the sign of a zero result is unspecified)
// d is a reference-layout array (n, nlev, ntr) of reals, instance index fastest, leading dimension n, the block's first
// instance at index 0 -- the shape of an output of mpdata_stats.h.  It is only read, and nothing outside it is.
#ifndef MPDATA_LEVEL_ADD_H
#define MPDATA_LEVEL_ADD_H
#include <hip/hip_runtime.h>

#include "mpdata_wm_walk.h"

// Plan layout.  j: the plan side of f exactly as wm_job(which = 0) makes it for tracers [first, first + j.ntr) (j.prv on
// the first of them, strides in 8-byte elements; j.ref is not used).  The kernel needs the storage layout only: element
// e = s * nlev + kk of column slot c of a tile, split into whole 128-byte lines and a rest (mpdata_layout.h).
//   sel: the block (mpdata_wm_walk.h).  A slot that is no instance of it keeps its bits (the partner half of a split
//     pair is stored back as it was loaded).  The one exception is the PHANTOM of an odd fp32 plan (include/mpdata_hip.h 3f):
//     it takes the increment of the last instance whenever the block holds that instance, and so stays its copy.
//     EVERY level a window of a windowed plan stores (owned or not) takes the increment of the tall level it stands
//     for, so that all stored copies of a tall level stay as consistent as they were.
struct MpdataLevelAddJob {
  MpdataLayoutJob j;
  MpdataBlockSel sel;
  const void* d;
  int clip;
};
// the grid covers the tiles the block touches
hipError_t mpdata_level_add_wm(const MpdataLevelAddJob& b, hipStream_t stream);

// Reference layout: f(ld, -2:nx+3, nlev, ntr) with elem_bytes = 4 or 8, instances [sl0, sl0 + n) of its ld; one thread
// per instance, 64-bit offsets.
hipError_t mpdata_level_add_ref(void* f, int elem_bytes, long long ld, long long sl0, long long n, int nx, int nlev, int ntr,
                                const void* d, int clip, hipStream_t stream);

#endif
