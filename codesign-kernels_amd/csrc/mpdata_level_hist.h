// mpdata_level_hist.h -- host interface of the per-level histograms of the tracers of f (mpdata_level_hist.hip;
// include/mpdata_hip.h 3ab): per instance sl of the block (b = sl - sl0), level k = 1 .. nlev, over the INTERIOR columns
// i = 1 .. nx, with c_i = f(i,k,tc) and v_i = f(i,k,t), every statement rounded once in the arrays' precision, in this
// association, no contraction, the comparisons plain compare-and-select:
//   e_j = edges[j] rounded once to the arrays' precision         j = 0 .. nb
//   m_i = the number of j in 0 .. nb with c_i > e_j              column i is in bin m_i - 1 when 1 <= m_i <= nb
//   cnt(b,k,j)    :  q = +0;  do i = 1, nx:  if column i in bin j:  q = q + 1
//   bsum(b,k,j,r) :  s = +0;  do i = 1, nx:  if column i in bin j:  s = s + v_i      (r = t - first, t in [first, first + ntr))
// A column that is in no bin, or in another, is SELECTED away, never multiplied away.  cnt (n, nlev, nb) and bsum (n, nlev,
// nb, ntr): reference layout, leading dimension n, the block's first instance at index 0.  f is only read and nothing
// outside cnt and bsum is written; halo columns and the tracers outside tc and the range are not read.
#ifndef MPDATA_LEVEL_HIST_H
#define MPDATA_LEVEL_HIST_H
#include <hip/hip_runtime.h>

#include "mpdata_wm_walk.h"

#define MPDATA_LEVEL_HIST_BINS 32   // MPDATA_LEVEL_HIST_MAX_BINS of include/mpdata_hip.h

// Plan layout.  j: the plan side of f exactly as wm_job(which = 0) makes it for ALL tracers of the plan; tc in [0, j.ntr),
// [first, first + ntr) inside it (ntr = 0 with a NULL bsum).  The grid and the lane-owned walk are those of
// mpdata_level_cond.h: (tile, 64-element slice), a lane owns one element and walks its interior column slots as linear
// streams, NB columns in flight, a value tracer at the signed 64-bit offset (t - tc) * prv_tstride from the tc stream.
// The edges travel in the job, by value: e[0 .. nb] as given, e[nb + 1 .. 32] = +inf (no c_i exceeds them, so m_i counts
// over a whole bin class without a test on nb).
//   The bins of a lane are REGISTERS: a compile-time array of the bin class NBC = 4, 8 or 16 (the least that holds the bins
//   of the walk; a walk carries at most 16 bins in fp64 and 8 in fp32 -- the largest classes without a spill of either
//   register file --, a call of more bins is a launch per GROUP of bins, each reading tc again): m_i by NBC + 1 compares,
//   then an unrolled chain of selects, s[j] = (m == j + 1) ? s[j] + v : s[j]; the counters are 32-bit integers, exact,
//   made reals at the store.  One walk per value tracer, each over the tc stream and the t stream (one stream for t ==
//   tc); the first walk also counts.  No LDS, no barrier, no cross-lane traffic.
// sel: the block (mpdata_wm_walk.h); W > 1: only the levels a window OWNS are read, each written to its tall level.
struct MpdataLevelHistJob {
  MpdataLayoutJob j;
  MpdataBlockSel sel;
  int tc;           // the binned tracer
  int first, ntr;   // the value tracers (bsum NULL: not looked at)
  int nb;           // bins, 1 .. MPDATA_LEVEL_HIST_BINS
  int nb_all;       // (set by the launcher: the bins of the call, of which a walk carries nb: the stride of a tracer in bsum)
  void* cnt;        // NULL: not wanted
  void* bsum;       // NULL: not wanted (one of the two is given)
  double e[MPDATA_LEVEL_HIST_BINS + 1];
};
// edges: nb + 1 HOST doubles, non-decreasing, no NaN (the caller checked); read before the call returns
hipError_t mpdata_level_hist_wm(MpdataLevelHistJob& b, const double* edges, hipStream_t stream);

// Reference layout: f(ld, -2:nx+3, nlev, ntr_all) with elem_bytes = 4 or 8, instances [sl0, sl0 + n) of its ld.  One thread
// per instance and level row, loops over i, 64-bit offsets: the same walk, groups of 8 bins.
hipError_t mpdata_level_hist_ref(const void* f, int elem_bytes, long long ld, long long sl0, long long n, int nx, int nlev, int ntr_all,
                                 int tc, int nb, const double* edges, void* cnt, void* bsum, int first, int ntr, hipStream_t stream);

#endif
