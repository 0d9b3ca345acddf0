// mpdata_scale_uw.hip -- one factor per instance multiplied into a velocity array, in place (include/mpdata_hip.h 3j,
// mpdata_scale_uw.h): a(sl, :, :) = a(sl, :, :) * s(sl - sl0) -- what a subcycled step needs (SAM's kurant: ncycle from
// the Courant number, then ncycle advections on u / ncycle, w / ncycle), the write side of mpdata_courant.hip.  A kernel
// of its own outside the run: nothing is fused into the plan kernels.
//   plan layout: the walk of mpdata_wm_walk.h over the column slots the array stores reads and writes it once as a
//     linear stream -- 512 bytes per wave and column, eight columns in flight -- with its factor in a register.
//   reference layout: one thread per instance, coalesced along sl, the loop over the columns.
// Built with -ffp-contract=off and IEEE NaN handling; every result is one rounded multiply, nothing here adds.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "mpdata_scale_uw.h"

namespace {

using namespace wm_walk;

// ncol elements p[0], p[step], ... of a lane := element * fv: all NB loads of a batch are issued before the first
// store (the index is clamped, not predicated: a conditional load would be waited for on its own; the clamped
// duplicates of the last column are loaded before that column is stored and are stored nowhere); the batch's tail is
// cut by wave-uniform conditions.  A half with on[h] false keeps the bits it was loaded with (no multiply); a lane
// with no half on stores nothing.
template <typename R2>
__device__ inline void march_scale(R2* p, const long long step, const int ncol, const typename Elem<R2>::R (&fv)[Elem<R2>::N],
                                   const bool (&on)[Elem<R2>::N]) {
  typedef Elem<R2> E;
  bool any = false;
#pragma unroll
  for (int h = 0; h < E::N; ++h) any = any || on[h];
  for (int c = 0; c < ncol; c += NB) {
    R2 v[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) v[u] = p[(long long)min(c + u, ncol - 1) * step];
    if (any) {
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        if (c + u < ncol) {
#pragma unroll
          for (int h = 0; h < E::N; ++h) {
            typename E::R& x = E::at(v[u], h);
            const typename E::R y = x * fv[h];
            x = on[h] ? y : x;
          }
          p[(long long)(c + u) * step] = v[u];
        }
      }
    }
  }
}

// Plan layout: a wave per (tile of the block, 64-element slice of the chunk), lane -> element e = s * nlev + kk.
// R2: one 8-byte element (double, or the float2 of two adjacent instances).
template <typename R2>
__global__ void __launch_bounds__(256) wm_scale_uw_kernel(const MpdataScaleUwJob b, const long long t0, const int ntile, const int nslice) {
  typedef Elem<R2> E;
  typedef typename E::R R;
  const MpdataLayoutJob& j = b.j;
  const int lane = threadIdx.x & 63;
  const long long wv = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wv >= (long long)ntile * nslice) return;
  const int slice = (int)(wv % nslice);
  const long long tile = t0 + wv / nslice;
  const int e0 = slice * 64 + lane;
  const bool act = e0 < j.chunk;
  const int e = act ? e0 : 0;   // (idle lanes of the last slice read element 0 and store nothing)
  const int s = e / j.nlev;
  const bool in_main = e < j.main_e;
  const long long cstep = in_main ? j.main_e : j.chunk - j.main_e;
  R2* p = static_cast<R2*>(j.prv) + tile * j.prv_tile_stride +
          (in_main ? e : (long long)j.ncol_p * j.main_e + (e - j.main_e)) + j.prv_col0 * cstep;   // the array's first column
  // the factor of every half: the instance the slot stands for
  const long long nslots = b.sel.ncrms * b.sel.W;   // slots that are an instance (a window of one)
  R fv[E::N];
  bool on[E::N];
#pragma unroll
  for (int h = 0; h < E::N; ++h) {
    long long q = (tile * j.slp + s) * E::N + h;
    if (E::N == 2 && (nslots & 1) && q == nslots) q = nslots - 1;   // the phantom half follows the plan's last slot
    const long long sl = b.sel.W > 1 ? q / b.sel.W : q;
    const bool ok = act && sl >= b.sel.sl0 && sl < b.sel.sl0 + b.sel.n;   // else: padding, the partner of a split pair, a neighbour in the tile
    on[h] = ok;
    fv[h] = ok ? static_cast<const R*>(b.s)[sl - b.sel.sl0] : (R)1;
  }
  bool any = false;
#pragma unroll
  for (int h = 0; h < E::N; ++h) any = any || on[h];
  if (__ballot(any) == 0) return;   // (a slice of a tile whose instances all lie outside the block)
  march_scale<R2>(p, cstep, j.ncols, fv, on);
}

// Reference layout: element (sl, column slot c, level k) at a + sl + ld * (c + ncols * k).  x: instances of the block,
// y: levels.
template <typename R>
__global__ void __launch_bounds__(256) ref_scale_uw_kernel(R* a, const long long ld, const long long sl0, const long long n, const int ncols,
                                                          const long long nlevs, const R* s) {
  const long long bi = (long long)blockIdx.x * 256 + threadIdx.x;
  if (bi >= n) return;
  const bool on[1] = {true};
  const R fv[1] = {s[bi]};
  for (long long k = blockIdx.y; k < nlevs; k += gridDim.y) march_scale<R>(a + (sl0 + bi) + ld * ((long long)ncols * k), ld, ncols, fv, on);
}

}  // namespace

hipError_t mpdata_scale_uw_wm(const MpdataScaleUwJob& b, hipStream_t stream) {
  WmGrid g;
  if (!b.s) return hipErrorInvalidValue;
  const hipError_t e = wm_block_grid(b.j, b.sel, 1, &g);
  return e != hipSuccess ? e : wm_block_launch(wm_scale_uw_kernel<double>, wm_scale_uw_kernel<float2>, b, g, stream);
}

hipError_t mpdata_scale_uw_ref(void* a, int elem_bytes, long long ld, long long sl0, long long n, int ncols, int nlevs,
                               const void* s, hipStream_t stream) {
  if (!a || !s || ld < 1 || sl0 < 0 || n < 1 || sl0 + n > ld || ncols < 1 || nlevs < 1) return hipErrorInvalidValue;
  dim3 grid, block(256);
  if (ref_block_grid(n, nlevs, &grid) != hipSuccess) return hipErrorInvalidValue;
  return ref_real(elem_bytes, [&](auto r) {
    typedef decltype(r) R;
    hipLaunchKernelGGL((ref_scale_uw_kernel<R>), grid, block, 0, stream, static_cast<R*>(a), ld, sl0, n, ncols, (long long)nlevs,
                       static_cast<const R*>(s));
    return hipGetLastError();
  });
}
