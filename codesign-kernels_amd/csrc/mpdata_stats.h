// mpdata_stats.h -- host interface of the level-statistics kernels (mpdata_stats.hip; include/mpdata_hip.h 3g):
// per tracer, instance and level the sum, the minimum and the maximum of f over the interior columns 1 .. nx.
//   sum: s = +0.0; s = s + f(sl, i, k) for i = 1 .. nx, in this order, in the precision of f (no multiplication:
//        the same bits in both variants); min / max: the bits of the chosen element.
// Outputs are reference-layout arrays (n, nlev_out, ntr) of reals, instance index fastest, leading dimension n, the
// block's first instance at index 0; any of the three may be NULL (skipped), not all.  Halo columns are never read.
#ifndef MPDATA_STATS_H
#define MPDATA_STATS_H
#include <hip/hip_runtime.h>

#include "mpdata_wm_walk.h"

// Plan layout.  j: the plan side of f exactly as wm_job(which = 0) makes it for tracers [first, first + j.ntr) (j.prv on
// the first of them, strides in 8-byte elements; j.ref is not used).  The kernel needs the storage layout only: element
// e = s * nlev + kk of column slot c of a tile, split into whole 128-byte lines and a rest (mpdata_layout.h).
//   sel: the block (mpdata_wm_walk.h).  Slots that are no instance of it reach no output; every window of a windowed
//     plan writes its OWNED levels to the tall level they stand for (owned levels are right after a run whatever the
//     seams hold).
struct MpdataStatsJob {
  MpdataLayoutJob j;
  MpdataBlockSel sel;
  void *sum, *mn, *mx;
};
// the grid covers the tiles the block touches
hipError_t mpdata_stats_wm(const MpdataStatsJob& b, hipStream_t stream);

// Reference layout: f(ld, -2:nx+3, nlev, ntr) with elem_bytes = 4 or 8, instances [sl0, sl0 + n) of its ld; one thread
// per instance, 64-bit offsets.
hipError_t mpdata_stats_ref(const void* f, int elem_bytes, long long ld, long long sl0, long long n, int nx, int nlev, int ntr,
                            void* sum, void* mn, void* mx, hipStream_t stream);

#endif
