// mpdata_cell_add.h -- host interface of the per-cell sources of f, in place (mpdata_cell_add.hip; include/mpdata_hip.h
// 3p): per instance sl of the block, tracer t, INTERIOR column i = 1 .. nx and level k = 1 .. nlev, every operation
// rounded once in the arrays' precision, in this association, no contraction:
//   p            = c * s(sl,i,k,t)
//   g            = f(i,k) + p;   clip: g = max(0, g)
//   dsum(sl,k,t) : a = +0; do i = 1, nx: a = a + (g - f_old(i,k))                        (NULL: skipped)
//   f(i,k)       = g
// s (n, nx, nlev, ntr), dsum (n, nlev, ntr): reference layout, leading dimension n, the block's first instance at index
// 0.  s is only read, and nothing outside it is; halo columns are neither read nor written.  c comes as a double for both
// precisions and is rounded once to the arrays' precision before use.
#ifndef MPDATA_CELL_ADD_H
#define MPDATA_CELL_ADD_H
#include <hip/hip_runtime.h>

#include "mpdata_wm_walk.h"

// Plan layout.  j: the plan side of f exactly as wm_job(which = 0) makes it for tracers [first, first + j.ntr) (j.prv on
// the first of them, strides in 8-byte elements; j.ref is not used).
//   s is read where it lies, as mpdata_sediment.h reads wp: a workgroup owns the whole tiles of a group of adjacent
//     8-byte elements of the instance axis (16: a row of s of the group is 128 bytes of fp64, 256 of fp32; fewer where two
//     buffers of two columns of the levels would not fit) and copies the group's rows of a column batch into one of TWO
//     LDS buffers as [column][unit][level].  Nothing of s goes to device memory.
//   sel: the block (mpdata_wm_walk.h).  A slot that is no instance of it keeps its bits (the partner half of a split
//     pair is stored back as it was loaded: neither the add nor the clip reaches it).  The PHANTOM of an odd fp32 plan
//     takes the result of the plan's last slot, its partner in the pair, whenever the block holds that instance (W > 1:
//     the kernel leaves the inner plan's phantom alone and the caller restores it behind the call).
//     W > 1 (windowed plans): only the levels a window OWNS are written, each with s of the tall level it stands for;
//     dsum is written by each level's owner.  The operator is pointwise: nothing outside the owned levels is read, the
//     caller need not refresh the seams in front, and marks them stale afterwards.
struct MpdataCellAddJob {
  MpdataLayoutJob j;
  MpdataBlockSel sel;
  const void* s;
  double c;
  int clip;
  void* dsum;
};
hipError_t mpdata_cell_add_wm(const MpdataCellAddJob& b, hipStream_t stream);

// Reference layout: f(ld, -2:nx+3, nlev, ntr) with elem_bytes = 4 or 8, instances [sl0, sl0 + n) of its ld.  One thread
// per instance and (level, tracer) row marching i, 64-bit offsets, in place: a thread reads and writes its own row only.
hipError_t mpdata_cell_add_ref(void* f, int elem_bytes, long long ld, long long sl0, long long n, int nx, int nlev, int ntr,
                               const void* s, double c, int clip, void* dsum, hipStream_t stream);

#endif
