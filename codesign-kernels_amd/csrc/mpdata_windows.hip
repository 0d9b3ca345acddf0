// mpdata_windows.hip -- the layout kernels of windowed plans (include/mpdata_hip.h 3e, mpdata_windows.h): a column of
// nz > 238 levels is W overlapping windows of nz_w <= 64 levels, each a pseudo-instance of an ordinary wave-major plan
// (pseudo-instance sl * W + h, one per tile: nz_w > 32).  Nothing here computes; the plan kernels never see a window.
//   split / merge: the LDS transpose of wm_block_kernel (mpdata_layout.hip) with a level offset -- a workgroup moves
//     the levels of ONE window of TI adjacent instances of one column: the tall reference side in row segments of TI
//     reals, the plan side in the contiguous column chunks of TI tiles.  Split writes every level a window holds,
//     merge reads every level and stores the owned ones, so every element of the tall array is written exactly once.
//   seam refresh: in place on the plan side, every non-owned level of a window := the value of the window that owns
//     it.  Sources are owned levels, destinations are non-owned ones: the two sets are disjoint, no store of this
//     kernel touches a byte another thread reads or writes, and no ordering is needed.
// E is ONE real as bits (fp32 plans hold pairs of adjacent pseudo-instances, which need not be two windows of one
// instance: W may be odd), so both sides move single reals, with vector loads and stores only.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "mpdata_windows.h"

namespace {

constexpr int TI = 32;   // instances per workgroup of split / merge: the LDS tile is nlev x (TI + 1) reals, <= 17 KB

// offset, in reals, of level kk (0-based) of column slot c of pseudo-instance q on the plan side (one pseudo-instance
// per tile; f, u, w: the whole 128-byte lines of a column chunk first, mpdata_layout.h)
__device__ inline long long prv_at(const MpdataLayoutJob& j, const int ipe, const long long q, const long long c, const int kk) {
  const long long t = q / ipe, half = q - t * ipe;
  const long long rem_e = j.chunk - j.main_e;
  const long long o = j.main_e == 0 ? c * j.chunk + kk
                                    : (kk < j.main_e ? c * j.main_e + kk : j.ncol_p * j.main_e + c * rem_e + (kk - j.main_e));
  return (t * j.prv_tile_stride + o) * ipe + half;
}

template <typename E, bool TO_PRIVATE>
__global__ void __launch_bounds__(256) window_convert_kernel(const MpdataWindowJob b, const int W) {
  extern __shared__ double lds_raw[];
  E* tile = reinterpret_cast<E*>(lds_raw);   // [nlev][TI + 1]
  const MpdataLayoutJob& j = b.j;
  constexpr int TP = TI + 1;
  const int tid = threadIdx.x;
  const int cs = blockIdx.y / W, h = blockIdx.y - cs * W, tr = blockIdx.z;
  const int nlev = j.nlev, ipe = b.ipe;
  int k0, nz_w, own0, own1;
  if (mpd_level_window(b.nz, h, &k0, &nz_w, &own0, &own1) != W || nz_w - 1 != nlev) return;   // (uniform: before the barrier)
  const int nel = nlev * TI;
  const long long b0 = (long long)blockIdx.x * TI;   // first instance of this workgroup, in the block
  E* ref = static_cast<E*>(j.ref) + (long long)tr * j.ref_tstride;
  E* prv = static_cast<E*>(j.prv) + (long long)tr * j.prv_tstride * ipe;
  const long long c = cs + j.prv_col0;
  auto ref_at = [&](const long long bi, const int kk) -> long long {
    return bi + b.n * ((long long)cs * j.ref_colmul + (long long)(k0 + kk) * j.ref_levmul);
  };
  // reference side: i -> (level, instance), a row segment per level; plan side: i -> (instance, level), a chunk per instance
  for (int i = tid; i < nel; i += 256) {
    int kk, t;
    if (TO_PRIVATE) { kk = i / TI; t = i - kk * TI; } else { t = i / nlev; kk = i - t * nlev; }
    const long long bi = b0 + t;
    if (bi < b.n) tile[kk * TP + t] = TO_PRIVATE ? ref[ref_at(bi, kk)] : prv[prv_at(j, ipe, (b.sl0 + bi) * W + h, c, kk)];
  }
  __syncthreads();
  for (int i = tid; i < nel; i += 256) {
    int kk, t;
    if (TO_PRIVATE) { t = i / nlev; kk = i - t * nlev; } else { kk = i / TI; t = i - kk * TI; }
    const long long bi = b0 + t;
    if (bi >= b.n) continue;
    if (TO_PRIVATE) prv[prv_at(j, ipe, (b.sl0 + bi) * W + h, c, kk)] = tile[kk * TP + t];
    else if (k0 + kk + 1 >= own0 && k0 + kk + 1 <= own1) ref[ref_at(bi, kk)] = tile[kk * TP + t];
  }
}

// A workgroup per (window of an instance, tracer): its threads walk (column slot, non-owned level).
template <typename E>
__global__ void __launch_bounds__(256) window_seams_kernel(const MpdataWindowJob b, const int W) {
  const MpdataLayoutJob& j = b.j;
  const long long q = blockIdx.x;            // pseudo-instance
  const long long sl = q / W;
  const int h = (int)(q - sl * W), tr = blockIdx.y, ipe = b.ipe;
  int k0, nz_w, own0, own1;
  if (mpd_level_window(b.nz, h, &k0, &nz_w, &own0, &own1) != W || nz_w - 1 != j.nlev) return;
  const int m = nz_w - 1;
  const int nlo = own0 - (k0 + 1), nhi = (k0 + m) - own1;   // non-owned levels below / above the owned range
  const int nno = nlo + nhi;
  E* prv = static_cast<E*>(j.prv) + (long long)tr * j.prv_tstride * ipe;
  for (int i = threadIdx.x; i < j.ncol_p * nno; i += 256) {
    const int c = i / nno, jj = i - c * nno;
    const int kk = jj < nlo ? jj : m - nno + jj;   // level of this window, 0-based
    const int k = k0 + kk + 1;                     // tall level
    int hh = h, s0 = k0, a0, a1, nw;
    if (jj < nlo) { do { --hh; mpd_level_window(b.nz, hh, &s0, &nw, &a0, &a1); } while (a0 > k); }
    else { do { ++hh; mpd_level_window(b.nz, hh, &s0, &nw, &a0, &a1); } while (a1 < k); }
    prv[prv_at(j, ipe, q, c, kk)] = prv[prv_at(j, ipe, sl * W + hh, c, k - s0 - 1)];
  }
}

// what both launches need of a job; W by the geometry
int check(const MpdataWindowJob& b) {
  const MpdataLayoutJob& j = b.j;
  int k0, nz_w, own0, own1;
  const int W = mpd_level_window(b.nz, 0, &k0, &nz_w, &own0, &own1);
  if (W < 2 || j.nlev != nz_w - 1 || j.slp != 1 || j.chunk != j.nlev || j.ntr < 1 || j.ntr > 65535 || j.ncols < 1 ||
      (b.ipe != 1 && b.ipe != 2) || j.main_e < 0 || j.main_e > j.chunk || !j.prv)
    return 0;
  if (b.sl0 < 0 || b.n < 1 || b.sl0 + b.n > b.ncrms || (b.ncrms * W + b.ipe - 1) / b.ipe != j.ntiles) return 0;   // (fp32, an odd number of windows: one phantom half)
  return W;
}

}  // namespace

hipError_t mpdata_window_convert(const MpdataWindowJob& b, bool to_private, hipStream_t stream) {
  const int W = check(b);
  if (!W || !b.j.ref || (long long)b.j.ncols * W > 65535 || b.j.prv_col0 + b.j.ncols > (b.j.main_e ? b.j.ncol_p : 3))
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)((b.n + TI - 1) / TI), (unsigned)(b.j.ncols * W), (unsigned)b.j.ntr), block(256);
  const size_t lds = (size_t)b.j.nlev * (TI + 1) * (8 / b.ipe);
  if (b.ipe == 1) {
    if (to_private) hipLaunchKernelGGL((window_convert_kernel<unsigned long long, true>), grid, block, lds, stream, b, W);
    else hipLaunchKernelGGL((window_convert_kernel<unsigned long long, false>), grid, block, lds, stream, b, W);
  } else {
    if (to_private) hipLaunchKernelGGL((window_convert_kernel<unsigned, true>), grid, block, lds, stream, b, W);
    else hipLaunchKernelGGL((window_convert_kernel<unsigned, false>), grid, block, lds, stream, b, W);
  }
  return hipGetLastError();
}

hipError_t mpdata_window_seams(const MpdataWindowJob& b, hipStream_t stream) {
  const int W = check(b);
  if (!W || b.sl0 != 0 || b.n != b.ncrms || b.ncrms * W > 2147483647LL || b.j.ncol_p < 1 || b.j.main_e == 0) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(b.ncrms * W), (unsigned)b.j.ntr), block(256);
  if (b.ipe == 1) hipLaunchKernelGGL((window_seams_kernel<unsigned long long>), grid, block, 0, stream, b, W);
  else hipLaunchKernelGGL((window_seams_kernel<unsigned>), grid, block, 0, stream, b, W);
  return hipGetLastError();
}
