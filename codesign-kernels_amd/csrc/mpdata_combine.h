// mpdata_combine.h -- host interface of the linear combination of tracers of f, in place (mpdata_combine.hip;
// include/mpdata_hip.h 3z): per instance sl of the block (b = sl - sl0), level k = 1 .. nlev and INTERIOR column
// i = 1 .. nx, with x_j = f_old(i,k,src[j]) (also where src[j] == dst), every statement rounded once in the arrays'
// precision, in this association, no contraction, comparisons plain compare-and-select:
//   nsrc >= 1:  v = coef ? coef(b,k,0) * x_0 : x_0
//               do j = 1, nsrc-1:  p = coef ? coef(b,k,j) * x_j : x_j ;  v = v + p
//               c0 given:  v = v + c0(b,k)
//   nsrc == 0:  v = c0(b,k)
//   clip     :  v = (v > 0) ? v : +0
//   f(i,k,dst) = v
//   sum(b,k) :  s = +0; do i = 1, nx: s = s + v(i)                                  (NULL: skipped)
// coef (n, nlev, nsrc), c0, sum (n, nlev): reference layout, leading dimension n, the block's first instance at index 0.
// coef and c0 are only read, and nothing outside the arrays is touched; halo columns and every tracer but dst are not
// written, tracers that are no source are not read.
#ifndef MPDATA_COMBINE_H
#define MPDATA_COMBINE_H
#include <hip/hip_runtime.h>

#include "mpdata_wm_walk.h"

#define MPDATA_COMBINE_NSRC 8   // MPDATA_COMBINE_MAX of include/mpdata_hip.h: the sources of a call at most

// Columns in flight per lane and source, by the number of sources (docs/EXPERIMENTS.md AJ: the candidates were timed):
// 8 to 24 eight-byte loads in flight per lane, so that no kernel needs more than 128 VGPRs (4 waves per SIMD) or any
// scratch.  MPDATA_COMBINE_HI_SERIAL != 0: five to eight sources are walked INSIDE a batch of MPDATA_COMBINE_NB_SERIAL
// columns, v[u] accumulated source by source with two sources' loads in flight; the order of the adds of a cell is j
// ascending in every form, so all forms give the same bits.
#ifndef MPDATA_COMBINE_NB_LO
#define MPDATA_COMBINE_NB_LO 8    // 0, 1 and 2 sources
#endif
#ifndef MPDATA_COMBINE_NB_MID
#define MPDATA_COMBINE_NB_MID 4   // 3 and 4 sources
#endif
#ifndef MPDATA_COMBINE_NB_HI
#define MPDATA_COMBINE_NB_HI 2    // 5 to 8 sources, fp32 plans (a lane carries two cells)
#endif
#ifndef MPDATA_COMBINE_NB_HI_F64
#define MPDATA_COMBINE_NB_HI_F64 3   // 5 to 8 sources, fp64 plans: 3.9 % faster than 2 at 8 sources, where fp32 is 1.5 % slower
#endif
#ifndef MPDATA_COMBINE_HI_SERIAL
#define MPDATA_COMBINE_HI_SERIAL 0
#endif
#ifndef MPDATA_COMBINE_NB_SERIAL
#define MPDATA_COMBINE_NB_SERIAL 8
#endif

// Plan layout.  j: the plan side of f exactly as wm_job(which = 0) makes it for ALL tracers of the plan (j.prv on tracer
// 0, strides in 8-byte elements; j.ref is not used); dst and every src[0 .. nsrc-1] in [0, j.ntr), sources may repeat
// and may be dst.
//   The grid runs over (tile, 64-element slice) of the tiles the block touches -- no tracer axis.  A lane owns one
//   element and walks its interior column slots (mpdata_wm_walk.h) as 1 + nsrc linear streams: the dst stream at
//   j.prv + dst * prv_tstride is the base, source j lies at the signed 64-bit offset (src[j] - dst) * prv_tstride from it
//   (mpdata_combine_wm fills off[] from src[]).  coef(b,k,*) and c0(b,k) of the lane's instance and level are in
//   registers per half, loaded once; sum is lane-local, accumulated in column order.  No LDS, no barrier: a lane touches
//   the columns of its own element only.  All loads of a batch of columns are issued before its first store, so a source
//   that is dst is read old.  The dst stream itself is LOADED only by a lane that must store a half back as it was (below).
//   sel: the block (mpdata_wm_walk.h).  A slot that is no instance of it keeps its bits (the partner half of a split
//     pair is stored back as it was loaded; a lane none of whose halves is in the block stores nothing).  The PHANTOM of
//     an odd fp32 plan takes the result of the plan's last slot, its partner in the pair, whenever the block holds that
//     instance (W > 1: the kernel leaves the inner plan's phantom alone and the caller restores it behind the call).
//     W > 1 (windowed plans): only the levels a window OWNS are read and written, each with coef and c0 of the tall
//     level it stands for; sum is written by each level's owner.  The caller need not refresh the seams in front, and
//     marks those of dst stale afterwards.
struct MpdataCombineJob {
  MpdataLayoutJob j;
  MpdataBlockSel sel;
  int dst, nsrc;
  int src[MPDATA_COMBINE_NSRC];
  long long off[MPDATA_COMBINE_NSRC];   // filled by mpdata_combine_wm
  const void* coef;                     // NULL: no multiply
  const void* c0;                       // NULL: nothing added (nsrc == 0: required)
  int clip;                             // != 0: v = (v > 0) ? v : +0
  void* sum;                            // NULL: not wanted
};
hipError_t mpdata_combine_wm(const MpdataCombineJob& b, hipStream_t stream);

// Reference layout: f(ld, -2:nx+3, nlev, ntr) with elem_bytes = 4 or 8, instances [sl0, sl0 + n) of its ld.  One thread
// per instance and level row, one loop over i, 64-bit offsets (every source row at a signed offset from the dst row), in
// place: a thread writes its own row of dst only and has read a cell's sources before it stores the cell.
hipError_t mpdata_combine_ref(void* f, int elem_bytes, long long ld, long long sl0, long long n, int nx, int nlev, int ntr, int dst,
                              int nsrc, const int* src, const void* coef, const void* c0, int clip, void* sum, hipStream_t stream);

#endif
