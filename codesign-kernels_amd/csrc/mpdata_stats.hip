// mpdata_stats.hip -- horizontal sum, minimum and maximum per level of f (include/mpdata_hip.h 3g, mpdata_stats.h):
// a reduction over the interior columns 1 .. nx, a kernel of its own outside the run (nothing is fused into the plan
// kernels, nothing is kept between calls, the result is a function of f alone).
//   plan layout: the walk of mpdata_wm_walk.h over the column slots 3 .. nx+2 reads f once as a linear stream -- 512
//     bytes per wave and column, eight columns in flight -- and keeps the three running values of every lane in
//     registers.
//   reference layout: one thread per instance, coalesced along sl, the loop over i.
// Built with -ffp-contract=off; the sum is the sequential one of the definition (s = +0.0; s = s + f_i), and nothing
// here multiplies.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "mpdata_stats.h"

namespace {

using namespace wm_walk;

template <typename R> struct Real;
template <> struct Real<double> {
  __device__ static double inf() { return __builtin_huge_val(); }
  __device__ static double lo(double a, double b) { return fmin(a, b); }
  __device__ static double hi(double a, double b) { return fmax(a, b); }
};
template <> struct Real<float> {
  __device__ static float inf() { return __builtin_huge_valf(); }
  __device__ static float lo(float a, float b) { return fminf(a, b); }
  __device__ static float hi(float a, float b) { return fmaxf(a, b); }
};

// nx values p[0], p[step], ... of every lane: all NB loads of a batch are issued before the first is used (the index
// is clamped, not predicated: a conditional load would be waited for on its own); the batch's tail is cut by
// wave-uniform conditions.  min / max start from +inf / -inf, so the result carries the bits of an element.
template <typename R2>
__device__ inline void march(const R2* p, const long long step, const int nx, typename Elem<R2>::R (&s)[Elem<R2>::N],
                             typename Elem<R2>::R (&lo)[Elem<R2>::N], typename Elem<R2>::R (&hi)[Elem<R2>::N]) {
  typedef Elem<R2> E;
  typedef Real<typename E::R> T;
#pragma unroll
  for (int h = 0; h < E::N; ++h) { s[h] = 0; lo[h] = T::inf(); hi[h] = -T::inf(); }
  for (int i = 0; i < nx; i += NB) {
    R2 v[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) v[u] = p[(long long)min(i + u, nx - 1) * step];
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      if (i + u < nx) {
#pragma unroll
        for (int h = 0; h < E::N; ++h) {
          const typename E::R x = E::get(v[u], h);
          s[h] = s[h] + x;
          lo[h] = T::lo(lo[h], x);
          hi[h] = T::hi(hi[h], x);
        }
      }
    }
  }
}

// Plan layout: a wave per (tracer, tile of the block, 64-element slice of the chunk), lane -> element e = s * nlev + kk.
// R2: one 8-byte element (double, or the float2 of two adjacent instances).
template <typename R2>
__global__ void __launch_bounds__(256) wm_level_stats_kernel(const MpdataStatsJob b, const long long t0, const int ntile, const int nslice) {
  typedef Elem<R2> E;
  typedef typename E::R R;
  const MpdataLayoutJob& j = b.j;
  const int lane = threadIdx.x & 63;
  const long long wv = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wv >= (long long)j.ntr * ntile * nslice) return;
  const int slice = (int)(wv % nslice);
  const long long tt = wv / nslice;
  const int tr = (int)(tt / ntile);
  const long long tile = t0 + tt % ntile;
  const int nlev = j.nlev, nx = j.ncol_p - 6;
  const int e0 = slice * 64 + lane;
  const bool act = e0 < j.chunk;
  const int e = act ? e0 : 0;   // (idle lanes of the last slice read element 0 and store nothing)
  const int s = e / nlev, kk = e - s * nlev;
  const bool in_main = e < j.main_e;
  const long long cstep = in_main ? j.main_e : j.chunk - j.main_e;
  const R2* p = static_cast<const R2*>(j.prv) + (long long)tr * j.prv_tstride + tile * j.prv_tile_stride +
                (in_main ? e : (long long)j.ncol_p * j.main_e + (e - j.main_e)) + 3 * cstep;   // column 1 = slot 3
  R acc[E::N], lo[E::N], hi[E::N];
  march<R2>(p, cstep, nx, acc, lo, hi);
  if (!act) return;
  const int nlev_out = b.sel.nz - 1;
#pragma unroll
  for (int h = 0; h < E::N; ++h) {
    const long long q = (tile * j.slp + s) * E::N + h;   // slot: instance, or pseudo-instance of a windowed plan
    long long sl = q;
    int k = kk;
    if (b.sel.W > 1) {
      sl = q / b.sel.W;
      int k0, nz_w, own0, own1;
      if (mpd_level_window(b.sel.nz, (int)(q - sl * b.sel.W), &k0, &nz_w, &own0, &own1) != b.sel.W) continue;
      k = k0 + kk;
      if (k + 1 < own0 || k + 1 > own1) continue;
    }
    if (sl < b.sel.sl0 || sl >= b.sel.sl0 + b.sel.n) continue;   // padding, phantom, the partner of a split pair, a neighbour in the tile
    const long long o = (sl - b.sel.sl0) + b.sel.n * (k + (long long)nlev_out * tr);
    if (b.sum) static_cast<R*>(b.sum)[o] = acc[h];
    if (b.mn) static_cast<R*>(b.mn)[o] = lo[h];
    if (b.mx) static_cast<R*>(b.mx)[o] = hi[h];
  }
}

// Reference layout: element (sl, column i, row r = level + nlev * tracer) at f + sl + ld * ((i + 2) + (nx + 6) * r).
// x: instances of the block, y: rows.
template <typename R>
__global__ void __launch_bounds__(256) ref_level_stats_kernel(const R* f, const long long ld, const long long sl0, const long long n,
                                                             const int nx, const long long rows, R* sum, R* mn, R* mx) {
  const long long bi = (long long)blockIdx.x * 256 + threadIdx.x;
  if (bi >= n) return;
  for (long long r = blockIdx.y; r < rows; r += gridDim.y) {
    R acc[1], lo[1], hi[1];
    march<R>(f + (sl0 + bi) + ld * ((long long)(nx + 6) * r + 3), ld, nx, acc, lo, hi);
    const long long o = bi + n * r;
    if (sum) sum[o] = acc[0];
    if (mn) mn[o] = lo[0];
    if (mx) mx[o] = hi[0];
  }
}

}  // namespace

hipError_t mpdata_stats_wm(const MpdataStatsJob& b, hipStream_t stream) {
  WmGrid g;
  if (!b.sum && !b.mn && !b.mx) return hipErrorInvalidValue;
  const hipError_t e = wm_block_grid(b.j, b.sel, b.j.ntr, &g);
  return e != hipSuccess ? e : wm_block_launch(wm_level_stats_kernel<double>, wm_level_stats_kernel<float2>, b, g, stream);
}

hipError_t mpdata_stats_ref(const void* f, int elem_bytes, long long ld, long long sl0, long long n, int nx, int nlev, int ntr,
                            void* sum, void* mn, void* mx, hipStream_t stream) {
  if (!f || ld < 1 || sl0 < 0 || n < 1 || sl0 + n > ld || nx < 1 || nlev < 1 || ntr < 1 || (!sum && !mn && !mx)) return hipErrorInvalidValue;
  const long long rows = (long long)nlev * ntr;
  dim3 grid, block(256);
  if (ref_block_grid(n, rows, &grid) != hipSuccess) return hipErrorInvalidValue;
  return ref_real(elem_bytes, [&](auto r) {
    typedef decltype(r) R;
    hipLaunchKernelGGL((ref_level_stats_kernel<R>), grid, block, 0, stream, static_cast<const R*>(f), ld, sl0, n, nx, rows, static_cast<R*>(sum),
                       static_cast<R*>(mn), static_cast<R*>(mx));
    return hipGetLastError();
  });
}
