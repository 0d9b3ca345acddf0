// mpdata_relax.hip -- relaxation of f to a level profile, in place (include/mpdata_hip.h 3r, mpdata_relax.h):
// f = f - c * (f - m) on the interior columns, with m a given target per level or the horizontal mean of f itself -- the
// damping layer under the top of a host model, nudging towards a profile.  A kernel of its own outside the run: nothing
// is fused into the plan kernels, nothing is kept between calls.
//   plan layout: the walk of mpdata_wm_walk.h over the column slots 3 .. nx+2, a lane per element, m and c in registers.
//     With a target: one walk that loads and stores f (the march of mpdata_level_add.hip with another update).  Without
//     one, two forms: KEPT, nx <= KEPT_NX = 32 -- all columns of the lane's element are loaded into registers, summed,
//     updated and stored, so f is loaded once (64 registers of data at nx = 32, five waves per SIMD) --, and RE-READ,
//     every other nx -- the summing walk of mpdata_stats.hip, one divide, then the updating walk over the same columns;
//     nothing of f stays in registers between the walks.  Both give the same bits.  A lane touches the columns of its
//     own element only, so there is no LDS, no barrier and no ordering to argue.
//   reference layout: one thread per instance and (level, tracer) row, coalesced along sl, two loops over i; in place.
// Built with -ffp-contract=off and IEEE divides: every operation of the definition is rounded once, in its association.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "mpdata_relax.h"

namespace {

using namespace wm_walk;

// the sum of nx values p[0], p[step], ... of every lane, s = +0; s = s + f_i: all NB loads of a batch are issued before
// the first is used (the index is clamped, not predicated); the batch's tail is cut by wave-uniform conditions.
template <typename R2>
__device__ inline void march_sum(const R2* p, const long long step, const int nx, typename Elem<R2>::R (&s)[Elem<R2>::N]) {
  typedef Elem<R2> E;
#pragma unroll
  for (int h = 0; h < E::N; ++h) s[h] = 0;
  for (int i = 0; i < nx; i += NB) {
    R2 v[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) v[u] = p[(long long)min(i + u, nx - 1) * step];
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      if (i + u < nx) {
#pragma unroll
        for (int h = 0; h < E::N; ++h) s[h] = s[h] + E::get(v[u], h);
      }
    }
  }
}

// nx elements p[0], p[step], ... of a lane := x - c * (x - m): all NB loads of a batch are issued before the first store
// (clamped duplicates of the last column are loaded before that column is stored and are stored nowhere).  A half with
// on[h] false keeps the bits it was loaded with; follow: the second half takes the first half's result (the phantom); a
// lane with no half on stores nothing.
template <typename R2>
__device__ inline void march_relax(R2* p, const long long step, const int nx, const typename Elem<R2>::R (&m)[Elem<R2>::N],
                                   const typename Elem<R2>::R (&cv)[Elem<R2>::N], const bool (&on)[Elem<R2>::N], const bool follow) {
  typedef Elem<R2> E;
  typedef typename E::R R;
  bool any = false;
#pragma unroll
  for (int h = 0; h < E::N; ++h) any = any || on[h];
  for (int i = 0; i < nx; i += NB) {
    R2 v[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) v[u] = p[(long long)min(i + u, nx - 1) * step];
    if (any) {
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        if (i + u < nx) {
#pragma unroll
          for (int h = 0; h < E::N; ++h) {
            R& x = E::at(v[u], h);
            const R d = x - m[h];
            const R pr = cv[h] * d;
            const R y = x - pr;
            x = on[h] ? y : x;
          }
          if (E::N == 2 && follow) E::at(v[u], E::N - 1) = E::get(v[u], 0);
          p[(long long)(i + u) * step] = v[u];
        }
      }
    }
  }
}

// The KEPT form of mean mode, nx <= KEPT_NX: the columns of the lane's element stay in registers between the sum and the
// update, so f is loaded once.  Fully unrolled and statically indexed (no scratch); the loads go out in groups of NB with
// the index clamped inside a group, the groups cut by wave-uniform conditions.  sum, mean and update are those of
// march_sum and march_relax, in the same order: the same bits.
constexpr int KEPT_NX = 32;
template <typename R2>
__device__ inline void march_kept(R2* p, const long long step, const int nx, const typename Elem<R2>::R (&cv)[Elem<R2>::N],
                                  const bool (&on)[Elem<R2>::N], const bool follow, typename Elem<R2>::R (&m)[Elem<R2>::N],
                                  typename Elem<R2>::R* const (&pm)[Elem<R2>::N]) {
  typedef Elem<R2> E;
  typedef typename E::R R;
  R2 v[KEPT_NX];
#pragma unroll
  for (int g = 0; g < KEPT_NX; g += NB) {
    if (g < nx) {
#pragma unroll
      for (int u = 0; u < NB; ++u) v[g + u] = p[(long long)min(g + u, nx - 1) * step];
    }
  }
  R s[E::N];
#pragma unroll
  for (int h = 0; h < E::N; ++h) s[h] = 0;
#pragma unroll
  for (int i = 0; i < KEPT_NX; ++i) {
    if (i < nx) {
#pragma unroll
      for (int h = 0; h < E::N; ++h) s[h] = s[h] + E::get(v[i], h);
    }
  }
  const R rnx = (R)nx;
  bool any = false;
#pragma unroll
  for (int h = 0; h < E::N; ++h) {
    m[h] = s[h] / rnx;
    if (pm[h]) *pm[h] = m[h];
    any = any || on[h];
  }
  if (!any) return;
#pragma unroll
  for (int i = 0; i < KEPT_NX; ++i) {
    if (i < nx) {
#pragma unroll
      for (int h = 0; h < E::N; ++h) {
        R& x = E::at(v[i], h);
        const R d = x - m[h];
        const R pr = cv[h] * d;
        const R y = x - pr;
        x = on[h] ? y : x;
      }
      if (E::N == 2 && follow) E::at(v[i], E::N - 1) = E::get(v[i], 0);
      p[(long long)i * step] = v[i];
    }
  }
}

// Plan layout: a wave per (tracer, tile of the block, 64-element slice of the chunk), lane -> element e = s * nlev + kk.
// R2: one 8-byte element (double, or the float2 of two adjacent slots); MEAN: no target, m is the mean of the lane's row;
// KEPT (mean mode, nx <= KEPT_NX): march_kept in the place of the two marches.
template <typename R2, bool MEAN, bool KEPT = false>
__device__ inline void wm_relax(const MpdataRelaxJob& b, const long long t0, const int ntile, const int nslice) {
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
  R2* p = static_cast<R2*>(j.prv) + (long long)tr * j.prv_tstride + tile * j.prv_tile_stride +
          (in_main ? e : (long long)j.ncol_p * j.main_e + (e - j.main_e)) + 3 * cstep;   // column 1 = slot 3
  // per half: the instance and the tall level the slot stands for, its factor and its place in target and mean
  const int nzm = b.sel.nz - 1;
  const long long nslots = b.sel.ncrms * b.sel.W;   // slots that are an instance (a window of one)
  R cv[E::N], m[E::N];
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
    const long long ob = ok ? (sl - b.sel.sl0) + b.sel.n * (long long)k : 0;
    o[h] = ob + b.sel.n * ((long long)nzm * tr);
    cv[h] = ok ? static_cast<const R*>(b.c)[ob] : (R)0;
    on[h] = ok && cv[h] != (R)0;
    m[h] = 0;
    if (!MEAN && ok) m[h] = static_cast<const R*>(b.target)[o[h]];
  }
  // the phantom half of an odd fp32 plan follows the plan's last slot, its partner in the element (W > 1: the caller
  // restores the inner plan's phantom behind the kernel)
  const bool follow = E::N == 2 && b.sel.W == 1 && (nslots & 1) && act && (tile * j.slp + s) * E::N + 1 == nslots && on[0];
  if (MEAN) {
    bool need = false;   // a row whose sum reaches a result
#pragma unroll
    for (int h = 0; h < E::N; ++h) need = need || (in[h] && (on[h] || b.mean));
    if (__ballot(need) == 0) return;
    if (KEPT) {
      R* pm[E::N];
#pragma unroll
      for (int h = 0; h < E::N; ++h) pm[h] = (b.mean && in[h]) ? static_cast<R*>(b.mean) + o[h] : nullptr;
      march_kept<R2>(p, cstep, nx, cv, on, follow, m, pm);
      return;
    }
    R acc[E::N];
    march_sum<R2>(p, cstep, nx, acc);
    const R rnx = (R)nx;   // exact: nx < 2^24
#pragma unroll
    for (int h = 0; h < E::N; ++h) m[h] = acc[h] / rnx;
  }
  if (b.mean) {
#pragma unroll
    for (int h = 0; h < E::N; ++h)
      if (in[h]) static_cast<R*>(b.mean)[o[h]] = m[h];
  }
  bool any = false;
#pragma unroll
  for (int h = 0; h < E::N; ++h) any = any || on[h];
  if (__ballot(any) == 0) return;   // (a slice whose elements all lie outside the block or have c == 0: nothing to load)
  march_relax<R2>(p, cstep, nx, m, cv, on, follow);
}
template <typename R2>
__global__ void __launch_bounds__(256) wm_relax_target_kernel(const MpdataRelaxJob b, const long long t0, const int ntile, const int nslice) {
  wm_relax<R2, false>(b, t0, ntile, nslice);
}
template <typename R2>
__global__ void __launch_bounds__(256) wm_relax_mean_kernel(const MpdataRelaxJob b, const long long t0, const int ntile, const int nslice) {
  wm_relax<R2, true>(b, t0, ntile, nslice);
}

template <typename R2>
__global__ void __launch_bounds__(256) wm_relax_kept_kernel(const MpdataRelaxJob b, const long long t0, const int ntile, const int nslice) {
  wm_relax<R2, true, true>(b, t0, ntile, nslice);
}

// Reference layout: element (sl, column i, row r = level + nlev * tracer) at f + sl + ld * ((i + 2) + (nx + 6) * r); c at
// bi + n * level, target and mean at bi + n * r.  x: instances of the block, y: rows.
template <typename R>
__global__ void __launch_bounds__(256) ref_relax_kernel(R* f, const long long ld, const long long sl0, const long long n, const int nx,
                                                       const int nlev, const long long rows, const R* c, const R* target, R* mean) {
  const long long bi = (long long)blockIdx.x * 256 + threadIdx.x;
  if (bi >= n) return;
  for (long long r = blockIdx.y; r < rows; r += gridDim.y) {
    R* const p = f + (sl0 + bi) + ld * ((long long)(nx + 6) * r + 3);   // column 1
    const R cv[1] = {c[bi + n * (r % nlev)]};
    const bool on[1] = {cv[0] != (R)0};
    R m[1];
    if (target) {
      m[0] = target[bi + n * r];
    } else {
      if (!on[0] && !mean) continue;
      R acc[1];
      march_sum<R>(p, ld, nx, acc);
      m[0] = acc[0] / (R)nx;
    }
    if (mean) mean[bi + n * r] = m[0];
    if (on[0]) march_relax<R>(p, ld, nx, m, cv, on, false);
  }
}

}  // namespace

hipError_t mpdata_relax_wm(const MpdataRelaxJob& b, hipStream_t stream) {
  WmGrid g;
  if (!b.c) return hipErrorInvalidValue;
  const hipError_t e = wm_block_grid(b.j, b.sel, b.j.ntr, &g);
  if (e != hipSuccess) return e;
  if (!b.target && b.j.ncol_p - 6 <= KEPT_NX)   // mean mode, the columns fit the registers: f is loaded once
    return wm_block_launch(wm_relax_kept_kernel<double>, wm_relax_kept_kernel<float2>, b, g, stream);
  return b.target ? wm_block_launch(wm_relax_target_kernel<double>, wm_relax_target_kernel<float2>, b, g, stream)
                  : wm_block_launch(wm_relax_mean_kernel<double>, wm_relax_mean_kernel<float2>, b, g, stream);
}

hipError_t mpdata_relax_ref(void* f, int elem_bytes, long long ld, long long sl0, long long n, int nx, int nlev, int ntr,
                            const void* c, const void* target, void* mean, hipStream_t stream) {
  if (!f || !c || ld < 1 || sl0 < 0 || n < 1 || sl0 + n > ld || nx < 1 || nlev < 1 || ntr < 1) return hipErrorInvalidValue;
  const long long rows = (long long)nlev * ntr;
  dim3 grid, block(256);
  if (ref_block_grid(n, rows, &grid) != hipSuccess) return hipErrorInvalidValue;
  return ref_real(elem_bytes, [&](auto r) {
    typedef decltype(r) R;
    hipLaunchKernelGGL((ref_relax_kernel<R>), grid, block, 0, stream, static_cast<R*>(f), ld, sl0, n, nx, nlev, rows,
                       static_cast<const R*>(c), static_cast<const R*>(target), static_cast<R*>(mean));
    return hipGetLastError();
  });
}
