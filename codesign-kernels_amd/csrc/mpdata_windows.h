// mpdata_windows.h -- tall columns as overlapping level windows (include/mpdata_hip.h 3e): the geometry, one function
// for host code and kernels alike, and the host interface of the window kernels (mpdata_windows.hip).
#ifndef MPDATA_WINDOWS_H
#define MPDATA_WINDOWS_H
#include <hip/hip_runtime.h>

#include "mpdata_layout.h"

// Window h of a column of nz levels (nzm = nz - 1 real levels, level nz the ghost level of w / rhow / flux).
//   Every window has the same m real levels (+ its own ghost level: a problem of nz_w = m + 1 levels), the tall
//   levels k0 + 1 .. k0 + m.  A window edge that is not an end of the column is ARTIFICIAL: the window clamps kb / kc
//   there and takes www = 0 above its top level, which spoils the first-pass value of the edge level, the limiter
//   ratios of the next one and the final value of the third.  A window therefore OWNS only levels that lie 3 or more
//   real levels inside its artificial edges: window levels 4 .. m - 3, consecutive windows at most m - 6 apart.
//     W    = 1                           nz <= 64 (the whole column)
//          = ceil((nzm - 6) / 57)        else: the fewest windows of m <= 63 levels
//     m    = ceil((nzm + 6 (W - 1)) / W)      the lowest windows that W of them can be (least duplicated work)
//     k0_h = floor(h (nzm - m) / (W - 1))     even spread: the first window on level 1, the last one ends on nzm, so
//                                             that its ghost level is the real level nz
//     own0 = 1 (h = 0), else k0_h + 4;   own1 = nzm (h = W - 1), else k0_{h+1} + 3
//   k0_{h+1} - k0_h <= ceil((nzm - m) / (W - 1)) <= m - 6 by the choice of m, hence own1 <= k0_h + m - 3.
// Returns W, or -1 for nz < 2 or h outside [0, W).  Levels are 1-based tall levels.
#if defined(__HIPCC__)
#define MPDW_HD __host__ __device__
#else
#define MPDW_HD
#endif
MPDW_HD inline int mpd_level_window(const int nz, const int h, int* k0, int* nz_w, int* own0, int* own1) {
  if (nz < 2) return -1;
  const int nzm = nz - 1;
  int W = 1, m = nzm;
  if (nz > 64) {
    W = (nzm - 6 + 56) / 57;
    m = (nzm + 6 * (W - 1) + W - 1) / W;
  }
  if (h < 0 || h >= W) return -1;
  const int D = nzm - m;
  const int a = W > 1 ? (int)((long long)h * D / (W - 1)) : 0;
  const int b = h + 1 < W ? (int)((long long)(h + 1) * D / (W - 1)) : 0;
  *k0 = a;
  *nz_w = m + 1;
  *own0 = h == 0 ? 1 : a + 4;
  *own1 = h == W - 1 ? nzm : b + 3;
  return W;
}

// One array of a windowed plan between the TALL reference layout and the inner wave-major plan of ncrms * W
// pseudo-instances (pseudo-instance sl * W + h = window h of instance sl; one pseudo-instance per tile).
//   j: the INNER plan's side exactly as wm_job makes it (j.nlev = nz_w - 1, j.slp = 1, strides in 8-byte elements);
//      j.ref: the tall array of the BLOCK of instances [sl0, sl0 + n), element (b, cs, level k) of tracer tr at
//      ref + tr*j.ref_tstride + b + n*(cs*ref_colmul + (k-1)*ref_levmul), in reals (whole plan: sl0 = 0, n = ncrms)
//   ipe: reals per 8-byte element of the private side: 1 (fp64), 2 (fp32: pairs of adjacent pseudo-instances)
struct MpdataWindowJob {
  MpdataLayoutJob j;
  long long sl0, n, ncrms;
  int ipe;
  int nz;   // of the tall column
};
// split (to_private: every level every window holds) / merge (the owned levels of every window)
hipError_t mpdata_window_convert(const MpdataWindowJob& b, bool to_private, hipStream_t stream);
// seam refresh, in place on the plan side: every non-owned level of every window := its owner's value, all ncol_p
// column slots, j.ntr tracers (a job of f)
hipError_t mpdata_window_seams(const MpdataWindowJob& b, hipStream_t stream);

#endif
