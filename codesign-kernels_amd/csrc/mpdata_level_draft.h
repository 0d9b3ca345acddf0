// mpdata_level_draft.h -- host interface of the per-level updraft / downdraft sampling of f by the vertical velocity w
// (mpdata_level_draft.hip; include/mpdata_hip.h 3ac): per instance sl of the block (b = sl - sl0), level k = 1 .. nzm, over
// the INTERIOR columns i = 1 .. nx, with c_i = f(i,k,tc) and v_i = f(i,k,t), every statement rounded once in the arrays'
// precision, in this association, no contraction, the comparisons plain compare-and-select:
//   wk1  = w(i,k+1) for k < nzm, +0 for k = nzm        (level nz of w is never read)
//   a    = w(i,k) + wk1;  wc = 0.5 * a
//   in_i = tc < 0 ? true : (lo ? c_i > lo(b,k) : true) and (hi ? c_i <= hi(b,k) : true)
//   class of column i, only where in_i:  UP (0): wc > wup   DOWN (1): wc < wdn   ENV (2): otherwise
//   cnt (b,k,c)    q = +0; do i: if class_i == c: q = q + 1
//   wsum(b,k,c)    s = +0; do i: if class_i == c: s = s + wc
//   fsum(b,k,c,r)  s = +0; do i: if class_i == c: s = s + v_i                 (r = t - first, t in [first, first + ntr))
//   wfsum(b,k,c,r) s = +0; do i: if class_i == c: p = wc * v_i; s = s + p
// A column outside a class is SELECTED away, never multiplied away.  cnt, wsum (n, nlev, 3) and fsum, wfsum (n, nlev, 3,
// ntr): reference layout, leading dimension n, the block's first instance at index 0.  f and w are only read and nothing
// outside the four outputs is written; halo columns and the tracers outside tc and the range are not read.
#ifndef MPDATA_LEVEL_DRAFT_H
#define MPDATA_LEVEL_DRAFT_H
#include <hip/hip_runtime.h>

#include "mpdata_wm_walk.h"

#define MPDATA_LEVEL_DRAFT_CLASSES 3   // UP, DOWN, ENV

// Plan layout.  j: the plan side of f exactly as wm_job(which = 0) makes it for ALL tracers of the plan; w: the plan side
// of w (wm_job(which = 2).prv: the geometry of f, another base, one array); tc in [-1, j.ntr), [first, first + ntr) inside
// the plan (ntr = 0 with fsum and wfsum NULL).  The grid and the lane-owned walk are those of mpdata_level_cond.h: (tile,
// 64-element slice), a lane owns one element and walks its interior column slots as linear streams; w(k) and w(k+1) are
// the two streams of mpdata_courant.hip (e1 = e + 1 through an address and a column stride of its own: e and e + 1 can
// lie on different sides of the main / rest split), a value tracer lies at the signed 64-bit offset (t - tc) *
// prv_tstride from the tc stream (tc < 0: from tracer 0, and no condition is loaded).
//   ONE form at every nx: the class of a column is formed again with every walk from w(k), w(k+1) and c_i, and a walk
//   carries a GROUP of 4, 2 or 1 value tracers (the most that is left), so the three class streams are read once per
//   group, not per tracer; the first walk also forms cnt and wsum.  The counters are 32-bit integers, exact, made reals at
//   the store.  Nothing of a column is kept between walks: no mask, no cache of wc.  No LDS, no barrier, no cross-lane
//   traffic.
// sel: the block (mpdata_wm_walk.h); W > 1: only the levels a window OWNS are read, each written to its tall level, with
// lo / hi of its tall level; wk1 is taken inside the window and is +0 at the window's top, which only the tall top owns.
struct MpdataLevelDraftJob {
  MpdataLayoutJob j;
  const void* w;
  MpdataBlockSel sel;
  int tc;             // the condition tracer, -1: none (lo and hi NULL)
  int first, ntr;     // the value tracers (fsum and wfsum NULL: not looked at)
  const void *lo, *hi;   // (n, nlev), either or both NULL
  double wup, wdn;    // wdn <= wup, no NaN (the caller checked); rounded once to the plan's precision in the kernel
  void *cnt, *wsum;   // (n, nlev, 3), NULL: not wanted
  void *fsum, *wfsum; // (n, nlev, 3, ntr), NULL: not wanted (one of the four is given)
};
hipError_t mpdata_level_draft_wm(const MpdataLevelDraftJob& b, hipStream_t stream);

// Reference layout: f(ld, -2:nx+3, nlev, ntr_all) and w(ld, -1:nx+2, nlev + 1) with elem_bytes = 4 or 8, instances [sl0,
// sl0 + n) of their ld.  One thread per instance and level row, loops over i, 64-bit offsets: the same walk, one value
// tracer a walk.  f may be NULL where tc < 0 and neither fsum nor wfsum is given.
hipError_t mpdata_level_draft_ref(const void* f, const void* w, int elem_bytes, long long ld, long long sl0, long long n, int nx, int nlev,
                                  int ntr_all, int tc, const void* lo, const void* hi, double wup, double wdn, void* cnt, void* wsum,
                                  void* fsum, void* wfsum, int first, int ntr, hipStream_t stream);

#endif
