// mpdata_level_add.hip -- per-level increments of f, in place (include/mpdata_hip.h 3i, mpdata_level_add.h):
// f(sl, i, k, t) = f(sl, i, k, t) + d(sl, k, t) on EVERY column slot i = -2 .. nx+3, optionally clipped at zero -- the
// large-scale forcing of a host model, the write side of the level statistics (mpdata_stats.hip).  A kernel of its own
// outside the run: nothing is fused into the plan kernels.
//   plan layout: the walk of mpdata_wm_walk.h over all nx + 6 column slots reads and writes f once as a linear stream
//     -- 512 bytes per wave and column, eight columns in flight -- with its increment in a register.
//   reference layout: one thread per instance, coalesced along sl, the loop over the columns.
// Built with -ffp-contract=off; every result is one rounded add (and the hardware max), nothing here multiplies.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "mpdata_level_add.h"

namespace {

using namespace wm_walk;

__device__ inline double pos(double a) { return fmax(a, 0.0); }
__device__ inline float pos(float a) { return fmaxf(a, 0.0f); }

// ncol elements p[0], p[step], ... of a lane := element + dv (clipped): all NB loads of a batch are issued before the
// first store (the index is clamped, not predicated: a conditional load would be waited for on its own; the clamped
// duplicates of the last column are loaded before that column is stored and are stored nowhere); the batch's tail is
// cut by wave-uniform conditions.  A half with on[h] false keeps the bits it was loaded with; a lane with no half on
// stores nothing.
template <typename R2>
__device__ inline void march_add(R2* p, const long long step, const int ncol, const typename Elem<R2>::R (&dv)[Elem<R2>::N],
                                 const bool (&on)[Elem<R2>::N], const bool clip) {
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
            const typename E::R y = x + dv[h];
            x = on[h] ? (clip ? pos(y) : y) : x;
          }
          p[(long long)(c + u) * step] = v[u];
        }
      }
    }
  }
}

// Plan layout: a wave per (tracer, tile of the block, 64-element slice of the chunk), lane -> element e = s * nlev + kk.
// R2: one 8-byte element (double, or the float2 of two adjacent instances).
template <typename R2>
__global__ void __launch_bounds__(256) wm_level_add_kernel(const MpdataLevelAddJob b, const long long t0, const int ntile, const int nslice) {
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
  const int nlev = j.nlev;
  const int e0 = slice * 64 + lane;
  const bool act = e0 < j.chunk;
  const int e = act ? e0 : 0;   // (idle lanes of the last slice read element 0 and store nothing)
  const int s = e / nlev, kk = e - s * nlev;
  const bool in_main = e < j.main_e;
  const long long cstep = in_main ? j.main_e : j.chunk - j.main_e;
  R2* p = static_cast<R2*>(j.prv) + (long long)tr * j.prv_tstride + tile * j.prv_tile_stride +
          (in_main ? e : (long long)j.ncol_p * j.main_e + (e - j.main_e));   // column slot 0
  // the increment of every half: the instance and the tall level the slot stands for
  const int nlev_d = b.sel.nz - 1;
  const long long nslots = b.sel.ncrms * b.sel.W;   // slots that are an instance (a window of one)
  R dv[E::N];
  bool on[E::N];
#pragma unroll
  for (int h = 0; h < E::N; ++h) {
    long long q = (tile * j.slp + s) * E::N + h;
    if (E::N == 2 && (nslots & 1) && q == nslots) q = nslots - 1;   // the phantom half follows the plan's last slot
    long long sl = q;
    int k = kk;
    bool ok = act;
    if (b.sel.W > 1) {
      sl = q / b.sel.W;
      int k0 = 0, nz_w, own0, own1;
      ok = ok && mpd_level_window(b.sel.nz, (int)(q - sl * b.sel.W), &k0, &nz_w, &own0, &own1) == b.sel.W;
      k = k0 + kk;
    }
    ok = ok && sl >= b.sel.sl0 && sl < b.sel.sl0 + b.sel.n && k < nlev_d;   // else: padding, the partner of a split pair, a neighbour in the tile
    on[h] = ok;
    dv[h] = ok ? static_cast<const R*>(b.d)[(sl - b.sel.sl0) + b.sel.n * (k + (long long)nlev_d * tr)] : (R)0;
  }
  bool any = false;
#pragma unroll
  for (int h = 0; h < E::N; ++h) any = any || on[h];
  if (__ballot(any) == 0) return;   // (a slice of a tile whose instances all lie outside the block)
  march_add<R2>(p, cstep, j.ncol_p, dv, on, b.clip != 0);
}

// Reference layout: element (sl, column slot c, row r = level + nlev * tracer) at f + sl + ld * (c + (nx + 6) * r).
// x: instances of the block, y: rows.
template <typename R>
__global__ void __launch_bounds__(256) ref_level_add_kernel(R* f, const long long ld, const long long sl0, const long long n, const int nx,
                                                           const long long rows, const R* d, const int clip) {
  const long long bi = (long long)blockIdx.x * 256 + threadIdx.x;
  if (bi >= n) return;
  const bool on[1] = {true};
  for (long long r = blockIdx.y; r < rows; r += gridDim.y) {
    const R dv[1] = {d[bi + n * r]};
    march_add<R>(f + (sl0 + bi) + ld * ((long long)(nx + 6) * r), ld, nx + 6, dv, on, clip != 0);
  }
}

}  // namespace

hipError_t mpdata_level_add_wm(const MpdataLevelAddJob& b, hipStream_t stream) {
  WmGrid g;
  if (!b.d) return hipErrorInvalidValue;
  const hipError_t e = wm_block_grid(b.j, b.sel, b.j.ntr, &g);
  return e != hipSuccess ? e : wm_block_launch(wm_level_add_kernel<double>, wm_level_add_kernel<float2>, b, g, stream);
}

hipError_t mpdata_level_add_ref(void* f, int elem_bytes, long long ld, long long sl0, long long n, int nx, int nlev, int ntr,
                                const void* d, int clip, hipStream_t stream) {
  if (!f || !d || ld < 1 || sl0 < 0 || n < 1 || sl0 + n > ld || nx < 1 || nlev < 1 || ntr < 1) return hipErrorInvalidValue;
  const long long rows = (long long)nlev * ntr;
  dim3 grid, block(256);
  if (ref_block_grid(n, rows, &grid) != hipSuccess) return hipErrorInvalidValue;
  return ref_real(elem_bytes, [&](auto r) {
    typedef decltype(r) R;
    hipLaunchKernelGGL((ref_level_add_kernel<R>), grid, block, 0, stream, static_cast<R*>(f), ld, sl0, n, nx, rows, static_cast<const R*>(d), clip);
    return hipGetLastError();
  });
}
