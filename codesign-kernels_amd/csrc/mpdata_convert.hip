// mpdata_convert.hip -- first-order, thresholded conversion between two tracers of f, in place (include/mpdata_hip.h 3t,
// mpdata_convert.h): d = r * max(a - q0, 0), optionally capped by max(a, 0), taken from tracer src and given to tracer
// dst (times a yield) on the interior columns -- autoconversion of cloud water into rain, a decay chain, a loss with a
// yield.  The first block call that sees two tracers of a cell.  A kernel of its own outside the run: nothing is fused
// into the plan kernels, nothing is kept between calls.
//   plan layout: the walk of mpdata_wm_walk.h over the column slots 3 .. nx+2, a lane per element, as TWO streams -- the
//     src tracer and, at a signed 64-bit offset from it, the dst tracer --, NB columns in flight on each; r, q0, y in
//     registers, dsum lane-local in column order.  A lane touches the columns of its own element only, so there is no
//     LDS, no barrier and no ordering to argue.
//   reference layout: one thread per instance and level row, coalesced along sl, one loop over i; in place.
// Built with -ffp-contract=off: every operation of the definition is rounded once, in its association; the comparisons
// are compare-and-select (NaN and -0 fall to the +0 branch), never fmax / fmin.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "mpdata_convert.h"

namespace {

using namespace wm_walk;

// the coefficients of one half of a lane's element
template <typename R>
struct Coef {
  R r, q0, y;
};

// one cell of the definition, statement by statement: xa (tracer src) and xc (tracer dst) are updated where on, else they
// keep the bits they came with; -> d
template <typename R>
__device__ inline R convert_cell(R& xa, R& xc, const Coef<R>& cf, const bool hasq, const bool hasy, const bool limit, const bool on) {
  const R a = xa, c = xc;
  R e = a;
  if (hasq) e = a - cf.q0;
  e = (e > (R)0) ? e : (R)0;
  R d = cf.r * e;
  if (limit) {
    const R m = (a > (R)0) ? a : (R)0;
    d = (d > m) ? m : d;
  }
  const R na = a - d;
  R g = d;
  if (hasy) g = cf.y * d;
  const R nc = c + g;
  xa = on ? na : a;
  xc = on ? nc : c;
  return d;
}

// nx elements p[0], p[step], ... (tracer src) and p[doff], p[doff + step], ... (tracer dst) of a lane: all 2 NB loads of
// a batch are issued before the first store (clamped duplicates of the last column are loaded before that column is
// stored and are stored nowhere).  A half with on[h] false keeps the bits it was loaded with in both tracers and adds
// nothing to s; follow: the second half takes the first half's results (the phantom); a lane with no half on stores
// nothing.  s[h]: s = +0; s = s + d(i), i ascending.
template <typename R2>
__device__ inline void march_convert(R2* p, const long long doff, const long long step, const int nx,
                                     const Coef<typename Elem<R2>::R> (&cf)[Elem<R2>::N], const bool hasq, const bool hasy, const bool limit,
                                     const bool (&on)[Elem<R2>::N], const bool follow, typename Elem<R2>::R (&s)[Elem<R2>::N]) {
  typedef Elem<R2> E;
  typedef typename E::R R;
  bool any = false;
#pragma unroll
  for (int h = 0; h < E::N; ++h) {
    any = any || on[h];
    s[h] = 0;
  }
  R2* const pd = p + doff;
  for (int i = 0; i < nx; i += NB) {
    R2 va[NB], vc[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) va[u] = p[(long long)min(i + u, nx - 1) * step];
#pragma unroll
    for (int u = 0; u < NB; ++u) vc[u] = pd[(long long)min(i + u, nx - 1) * step];
    if (any) {
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        if (i + u < nx) {
#pragma unroll
          for (int h = 0; h < E::N; ++h) {
            const R d = convert_cell<R>(E::at(va[u], h), E::at(vc[u], h), cf[h], hasq, hasy, limit, on[h]);
            if (on[h]) s[h] = s[h] + d;
          }
          if (E::N == 2 && follow) {
            E::at(va[u], E::N - 1) = E::get(va[u], 0);
            E::at(vc[u], E::N - 1) = E::get(vc[u], 0);
          }
          p[(long long)(i + u) * step] = va[u];
          pd[(long long)(i + u) * step] = vc[u];
        }
      }
    }
  }
}

// Plan layout: a wave per (tile of the block, 64-element slice of the chunk), lane -> element e = s * nlev + kk.
// R2: one 8-byte element (double, or the float2 of two adjacent slots).
template <typename R2>
__global__ void __launch_bounds__(256) wm_convert_kernel(const MpdataConvertJob b, const long long t0, const int ntile, const int nslice) {
  typedef Elem<R2> E;
  typedef typename E::R R;
  const MpdataLayoutJob& j = b.j;
  const int lane = threadIdx.x & 63;
  const long long wv = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wv >= (long long)ntile * nslice) return;
  const int slice = (int)(wv % nslice);
  const long long tile = t0 + wv / nslice;
  const int nlev = j.nlev, nx = j.ncol_p - 6;
  const int e0 = slice * 64 + lane;
  const bool act = e0 < j.chunk;
  const int e = act ? e0 : 0;   // (idle lanes of the last slice read element 0 and store nothing)
  const int s = e / nlev, kk = e - s * nlev;
  const bool in_main = e < j.main_e;
  const long long cstep = in_main ? j.main_e : j.chunk - j.main_e;
  R2* p = static_cast<R2*>(j.prv) + (long long)b.src * j.prv_tstride + tile * j.prv_tile_stride +
          (in_main ? e : (long long)j.ncol_p * j.main_e + (e - j.main_e)) + 3 * cstep;   // column 1 = slot 3
  const long long doff = (long long)(b.dst - b.src) * j.prv_tstride;                     // signed: dst < src walks back
  // per half: the instance and the tall level the slot stands for, its coefficients and its place in dsum
  const int nzm = b.sel.nz - 1;
  const long long nslots = b.sel.ncrms * b.sel.W;   // slots that are an instance (a window of one)
  Coef<R> cf[E::N];
  bool in[E::N], on[E::N];
  long long o[E::N];
#pragma unroll
  for (int h = 0; h < E::N; ++h) {
    const long long q = (tile * j.slp + s) * E::N + h;
    long long sl = q;
    int k = kk;
    bool ok = act;
    if (b.sel.W > 1) {
      sl = q / b.sel.W;
      int k0 = 0, nz_w, own0 = 1, own1 = 0;
      ok = ok && mpd_level_window(b.sel.nz, (int)(q - sl * b.sel.W), &k0, &nz_w, &own0, &own1) == b.sel.W;
      k = k0 + kk;
      ok = ok && k + 1 >= own0 && k + 1 <= own1;   // the level's owner alone reads and writes it
    }
    // else: padding, the phantom, the partner of a split pair, a neighbour in the tile
    ok = ok && sl >= b.sel.sl0 && sl < b.sel.sl0 + b.sel.n && k < nzm;
    in[h] = ok;
    o[h] = ok ? (sl - b.sel.sl0) + b.sel.n * (long long)k : 0;
    cf[h].r = ok ? static_cast<const R*>(b.r)[o[h]] : (R)0;
    on[h] = ok && cf[h].r != (R)0;
    cf[h].q0 = (b.q0 && ok) ? static_cast<const R*>(b.q0)[o[h]] : (R)0;
    cf[h].y = (b.y && ok) ? static_cast<const R*>(b.y)[o[h]] : (R)1;
  }
  // the phantom half of an odd fp32 plan follows the plan's last slot, its partner in the element (W > 1: the caller
  // restores the inner plan's phantom behind the kernel)
  const bool follow = E::N == 2 && b.sel.W == 1 && (nslots & 1) && act && (tile * j.slp + s) * E::N + 1 == nslots && on[0];
  bool any = false;
#pragma unroll
  for (int h = 0; h < E::N; ++h) any = any || on[h];
  R acc[E::N];
#pragma unroll
  for (int h = 0; h < E::N; ++h) acc[h] = 0;
  // (a slice whose elements all lie outside the block or have r == 0: nothing to load)
  if (__ballot(any) != 0) march_convert<R2>(p, doff, cstep, nx, cf, b.q0 != nullptr, b.y != nullptr, b.limit != 0, on, follow, acc);
  if (b.dsum) {
#pragma unroll
    for (int h = 0; h < E::N; ++h)
      if (in[h]) static_cast<R*>(b.dsum)[o[h]] = acc[h];
  }
}

// Reference layout: element (sl, column i, level k, tracer t) at f + sl + ld * ((i + 2) + (nx + 6) * (k + nlev * t)); r,
// q0, y, dsum at bi + n * k.  x: instances of the block, y: levels.
template <typename R>
__global__ void __launch_bounds__(256) ref_convert_kernel(R* f, const long long ld, const long long sl0, const long long n, const int nx,
                                                         const int nlev, const int src, const int dst, const R* r, const R* q0, const R* y,
                                                         const int limit, R* dsum) {
  const long long bi = (long long)blockIdx.x * 256 + threadIdx.x;
  if (bi >= n) return;
  const long long doff = ld * ((long long)(nx + 6) * nlev * (dst - src));   // signed
  for (long long k = blockIdx.y; k < nlev; k += gridDim.y) {
    R* const p = f + (sl0 + bi) + ld * ((long long)(nx + 6) * (k + (long long)nlev * src) + 3);   // column 1 of tracer src
    const long long o = bi + n * k;
    const Coef<R> cf = {r[o], q0 ? q0[o] : (R)0, y ? y[o] : (R)1};
    R acc = 0;
    if (cf.r != (R)0) {
      for (int i = 0; i < nx; ++i) {
        R xa = p[i * ld], xc = p[i * ld + doff];
        const R d = convert_cell<R>(xa, xc, cf, q0 != nullptr, y != nullptr, limit != 0, true);
        p[i * ld] = xa;
        p[i * ld + doff] = xc;
        acc = acc + d;
      }
    }
    if (dsum) dsum[o] = acc;
  }
}

}  // namespace

hipError_t mpdata_convert_wm(const MpdataConvertJob& b, hipStream_t stream) {
  WmGrid g;
  if (!b.r || b.src < 0 || b.dst < 0 || b.src >= b.j.ntr || b.dst >= b.j.ntr || b.src == b.dst) return hipErrorInvalidValue;
  const hipError_t e = wm_block_grid(b.j, b.sel, 1, &g);
  if (e != hipSuccess) return e;
  return wm_block_launch(wm_convert_kernel<double>, wm_convert_kernel<float2>, b, g, stream);
}

hipError_t mpdata_convert_ref(void* f, int elem_bytes, long long ld, long long sl0, long long n, int nx, int nlev, int ntr, int src,
                              int dst, const void* r, const void* q0, const void* y, int limit, void* dsum, hipStream_t stream) {
  if (!f || !r || ld < 1 || sl0 < 0 || n < 1 || sl0 + n > ld || nx < 1 || nlev < 1 || ntr < 2) return hipErrorInvalidValue;
  if (src < 0 || dst < 0 || src >= ntr || dst >= ntr || src == dst) return hipErrorInvalidValue;
  dim3 grid, block(256);
  if (ref_block_grid(n, nlev, &grid) != hipSuccess) return hipErrorInvalidValue;
  return ref_real(elem_bytes, [&](auto x) {
    typedef decltype(x) R;
    hipLaunchKernelGGL((ref_convert_kernel<R>), grid, block, 0, stream, static_cast<R*>(f), ld, sl0, n, nx, nlev, src, dst,
                       static_cast<const R*>(r), static_cast<const R*>(q0), static_cast<const R*>(y), limit, static_cast<R*>(dsum));
    return hipGetLastError();
  });
}
