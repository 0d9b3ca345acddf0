// mpdata_courant.hip -- outflow Courant number of the velocities per level and per instance (include/mpdata_hip.h 3h,
// mpdata_courant.h): the coefficient 1 - c of f(i,k) in the routine's upwind pass, a reduction over the interior columns
// 1 .. nx in a kernel of its own outside the run (nothing is fused into the plan kernels, nothing is kept between calls).
//   plan layout: the walk of mpdata_wm_walk.h, as the level statistics (mpdata_stats.hip) -- here the linear streams
//     of two arrays, u and w; u(i+1) is the lane's next column and is carried
//     over, w(k+1) is element e + 1 of the same column, loaded through an address of its own (e and e + 1 can lie on
//     different sides of the main / rest split of a chunk; the lines are the ones the wave has just asked for).
//   reference layout: one thread per instance, coalesced along sl, the loop over i.
// Built with -ffp-contract=off: every operation of the definition is rounded once, in the definition's association.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "mpdata_courant.h"

namespace {

using namespace wm_walk;

template <typename R> struct Real;
template <> struct Real<double> {
  typedef unsigned long long U;
  __device__ static double lo(double a, double b) { return fmin(a, b); }
  __device__ static double hi(double a, double b) { return fmax(a, b); }
  __device__ static double abs(double a) { return fabs(a); }
  __device__ static U bits(double a) { return (U)__double_as_longlong(a); }
};
template <> struct Real<float> {
  typedef unsigned int U;
  __device__ static float lo(float a, float b) { return fminf(a, b); }
  __device__ static float hi(float a, float b) { return fmaxf(a, b); }
  __device__ static float abs(float a) { return fabsf(a); }
  __device__ static U bits(float a) { return __float_as_uint(a); }
};

// the definition; the sign is cleared last (a, b and c can come out as -0.0 from signed zeros in u, w)
template <typename R>
__device__ inline R courant(const R u0, const R u1, const R w0, const R w1, const R iadz, const R irho) {
  typedef Real<R> T;
  const R a = T::hi((R)0, u1) - T::lo((R)0, u0);
  const R b = T::hi((R)0, w1) - T::lo((R)0, w0);
  return T::abs((a + b * iadz) * irho);
}

// The max over i = 1 .. nx of every lane: pu on u(1), pw on w(1) of level k, pw1 on w(1) of level k + 1 (top: there is
// none, pw1 = pw and +0 is taken), column strides su (u, w) and sw1.  All loads of a batch are issued before the first
// is used (the index is clamped, not predicated); the batch's tail is cut by wave-uniform conditions.
template <typename R2>
__device__ inline void march(const R2* pu, const R2* pw, const R2* pw1, const long long su, const long long sw1, const int nx,
                             const bool top, const typename Elem<R2>::R (&iadz)[Elem<R2>::N],
                             const typename Elem<R2>::R (&irho)[Elem<R2>::N], typename Elem<R2>::R (&m)[Elem<R2>::N]) {
  typedef Elem<R2> E;
  typedef typename E::R R;
#pragma unroll
  for (int h = 0; h < E::N; ++h) m[h] = 0;
  R2 uc = pu[0];
  for (int i = 0; i < nx; i += NB) {
    R2 un[NB], wv[NB], wn[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const long long c = min(i + u, nx - 1);
      un[u] = pu[(c + 1) * su];
      wv[u] = pw[c * su];
      wn[u] = pw1[c * sw1];
    }
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      if (i + u < nx) {
#pragma unroll
        for (int h = 0; h < E::N; ++h) {
          const R w1 = top ? (R)0 : E::get(wn[u], h);
          m[h] = Real<R>::hi(m[h], courant<R>(E::get(uc, h), E::get(un[u], h), E::get(wv[u], h), w1, iadz[h], irho[h]));
        }
        uc = un[u];
      }
    }
  }
}

// Plan layout: a wave per (tile of the block, 64-element slice of the chunk), lane -> element e = s * nlev + kk.
// R2: one 8-byte element (double, or the float2 of two adjacent instances).
template <typename R2>
__global__ void __launch_bounds__(256) wm_courant_kernel(const MpdataCourantJob b, const long long t0, const int ntile, const int nslice) {
  typedef Elem<R2> E;
  typedef typename E::R R;
  typedef typename Real<R>::U U;
  const MpdataLayoutJob& j = b.j;
  const int lane = threadIdx.x & 63;
  const long long wv = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wv >= (long long)ntile * nslice) return;   // (wave-uniform: the shuffles below see whole waves)
  const int slice = (int)(wv % nslice);
  const long long tile = t0 + wv / nslice;
  const int nlev = j.nlev, nx = j.ncol_p - 6;
  const int e0 = slice * 64 + lane;
  const bool act = e0 < j.chunk;
  const int e = act ? e0 : 0;   // (idle lanes of the last slice read element 0 and reach no output)
  const int s = e / nlev, kk = e - s * nlev;
  const bool top = kk + 1 == nlev;
  const int e1 = top ? e : e + 1;
  const long long rem_e = j.chunk - j.main_e;
  const bool main0 = e < j.main_e, main1 = e1 < j.main_e;
  const long long su = main0 ? j.main_e : rem_e, sw1 = main1 ? j.main_e : rem_e;
  const long long tb = tile * j.prv_tile_stride;
  const long long o0 = tb + (main0 ? e : (long long)j.ncol_p * j.main_e + (e - j.main_e)) + (1 + j.prv_col0 + 1) * su;     // column 1
  const long long o1 = tb + (main1 ? e1 : (long long)j.ncol_p * j.main_e + (e1 - j.main_e)) + (1 + j.prv_col0 + 1) * sw1;
  const R2 rho2 = static_cast<const R2*>(b.rho)[tile * b.kc_tile_stride + e];
  const R2 adz2 = static_cast<const R2*>(b.adz)[tile * b.kc_tile_stride + e];
  R iadz[E::N], irho[E::N], m[E::N];
#pragma unroll
  for (int h = 0; h < E::N; ++h) {
    iadz[h] = (R)1 / E::get(adz2, h);
    irho[h] = (R)1 / E::get(rho2, h);
  }
  march<R2>(static_cast<const R2*>(j.prv) + o0, static_cast<const R2*>(b.w) + o0, static_cast<const R2*>(b.w) + o1, su, sw1, nx, top,
            iadz, irho, m);
  const int nlev_out = b.sel.nz - 1;
#pragma unroll
  for (int h = 0; h < E::N; ++h) {
    const long long q = (tile * j.slp + s) * E::N + h;   // slot: instance, or pseudo-instance of a windowed plan
    long long sl = q;
    int k = kk;
    bool inst = act, owned = true;
    if (b.sel.W > 1) {
      sl = q / b.sel.W;
      int k0 = 0, nz_w, own0 = 1, own1 = 0;
      if (mpd_level_window(b.sel.nz, (int)(q - sl * b.sel.W), &k0, &nz_w, &own0, &own1) != b.sel.W) inst = false;
      k = k0 + kk;
      owned = k + 1 >= own0 && k + 1 <= own1;
    }
    // padding, phantom, the partner of a split pair, a neighbour in the tile: no output
    if (sl < b.sel.sl0 || sl >= b.sel.sl0 + b.sel.n) inst = false;
    const bool st = inst && owned;
    if (st && b.clev) static_cast<R*>(b.clev)[(sl - b.sel.sl0) + b.sel.n * k] = m[h];
    if (b.cinst) {
      // the lanes of one instance are consecutive: a suffix max inside the instance, then one atomic by its first lane
      R v = st ? m[h] : (R)0;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const R o = __shfl_down(v, d, 64);
        if (lane + d < 64 && kk + d < nlev) v = Real<R>::hi(v, o);
      }
      if (inst && (lane == 0 || kk == 0)) atomicMax(static_cast<U*>(b.cinst) + (sl - b.sel.sl0), Real<R>::bits(v));
    }
  }
}

// Reference layout: u (sl, column i, level k) at u + sl + ld * ((i + 1) + (nx + 5) * (k - 1)), w with nx + 4 columns, rho and
// adz at sl + ld * (k - 1).  x: instances of the block, y: levels.  Level nz of w is never read.
template <typename R>
__global__ void __launch_bounds__(256) ref_courant_kernel(const R* u, const R* w, const R* rho, const R* adz, const long long ld,
                                                          const long long sl0, const long long n, const int nx, const int nzm, R* clev,
                                                          typename Real<R>::U* cinst) {
  const long long bi = (long long)blockIdx.x * 256 + threadIdx.x;
  if (bi >= n) return;
  const long long sl = sl0 + bi;
  R best = 0;
  for (long long k = blockIdx.y; k < nzm; k += gridDim.y) {
    const bool top = k + 1 == nzm;
    const R* pw = w + sl + ld * ((long long)(nx + 4) * k + 2);
    const R iadz[1] = {(R)1 / adz[sl + ld * k]}, irho[1] = {(R)1 / rho[sl + ld * k]};
    R m[1];
    march<R>(u + sl + ld * ((long long)(nx + 5) * k + 2), pw, top ? pw : pw + ld * (nx + 4), ld, ld, nx, top, iadz, irho, m);
    if (clev) clev[bi + n * k] = m[0];
    best = Real<R>::hi(best, m[0]);
  }
  if (cinst) atomicMax(cinst + bi, Real<R>::bits(best));
}

}  // namespace

hipError_t mpdata_courant_wm(const MpdataCourantJob& b, hipStream_t stream) {
  WmGrid g;
  if (!b.w || !b.rho || !b.adz || b.j.prv_col0 != 1 || b.kc_tile_stride < b.j.chunk || (!b.clev && !b.cinst)) return hipErrorInvalidValue;
  hipError_t e = wm_block_grid(b.j, b.sel, 1, &g);
  if (e == hipSuccess && b.cinst) e = hipMemsetAsync(b.cinst, 0, (size_t)b.sel.n * (8 / b.sel.ipe), stream);
  return e != hipSuccess ? e : wm_block_launch(wm_courant_kernel<double>, wm_courant_kernel<float2>, b, g, stream);
}

hipError_t mpdata_courant_ref(const void* u, const void* w, const void* rho, const void* adz, int elem_bytes, long long ld,
                              long long sl0, long long n, int nx, int nz, void* clev, void* cinst, hipStream_t stream) {
  if (!u || !w || !rho || !adz || ld < 1 || sl0 < 0 || n < 1 || sl0 + n > ld || nx < 1 || nz < 2 || (!clev && !cinst) ||
      (elem_bytes != 4 && elem_bytes != 8))
    return hipErrorInvalidValue;
  const int nzm = nz - 1;
  dim3 grid, block(256);
  if (ref_block_grid(n, nzm, &grid) != hipSuccess) return hipErrorInvalidValue;
  if (cinst) {
    const hipError_t e = hipMemsetAsync(cinst, 0, (size_t)n * elem_bytes, stream);
    if (e != hipSuccess) return e;
  }
  return ref_real(elem_bytes, [&](auto r) {
    typedef decltype(r) R;
    hipLaunchKernelGGL((ref_courant_kernel<R>), grid, block, 0, stream, static_cast<const R*>(u), static_cast<const R*>(w),
                       static_cast<const R*>(rho), static_cast<const R*>(adz), ld, sl0, n, nx, nzm, static_cast<R*>(clev),
                       static_cast<typename Real<R>::U*>(cinst));
    return hipGetLastError();
  });
}
