// mpdata_diffuse.hip -- eddy diffusion of f, in place (include/mpdata_hip.h 3l, mpdata_diffuse.h): the sibling of the
// routine in a host model's time loop (SAM's diffuse_scalar2D), a Jacobi update of the interior columns from x-fluxes
// Fx and z-fluxes Fz of the OLD field.  The one block call that is a stencil: neighbours along x are the column walk of
// mpdata_wm_walk.h, neighbours along k are the lane axis of the plan layout.  A kernel of its own outside the run:
// nothing is fused into the plan kernels, nothing is kept between calls.
//   plan layout: a wave per 64-element slice of a tile's column chunk, lane -> element e = s * nlev + kk, walks the
//     interior columns as linear streams, NB columns in flight; old f(i), tkh(i) and Fx(i-1) are carried in registers
//     from column to column, so f is read once and written once.  f(i,k+-1) and tkh(i,k+-1) are elements e +- 1 of the
//     same column: inside a wave they come by a shuffle, selected only while kk +- 1 stays inside the instance; lane 0
//     and lane 63 load theirs from the neighbour slice.  The update is in place and an instance above 64 levels is
//     several slices, so: a WORKGROUP OWNS WHOLE TILES (every slot of an instance is in one workgroup; no workgroup
//     reads what another writes), and per batch every load -- the batch's look-ahead column and the edge neighbours of
//     the columns about to be stored -- is issued before a __syncthreads(), every store after it.  A batch stores
//     columns c .. c+NB-1; the loads of the next batch touch columns >= c+NB only, so one barrier per batch orders all
//     of it: the barrier a wave passes before it stores batch b is passed by every wave after its loads of batch b.
//   reference layout: one thread per instance and (level, tracer) row, coalesced along sl.  Rows of different levels
//     belong to threads of different workgroups, so the new interior goes to a scratch array and a second kernel on
//     the same stream copies it into f: the kernel boundary is the order.
// Built with -ffp-contract=off and IEEE divides: every operation of the definition is rounded once, in its association.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "mpdata_diffuse.h"

namespace {

using namespace wm_walk;

__device__ inline double lane_up(const double v) { return __shfl_up(v, 1); }      // the value of lane - 1
__device__ inline double lane_down(const double v) { return __shfl_down(v, 1); }  // the value of lane + 1
__device__ inline float2 lane_up(const float2 v) { return make_float2(__shfl_up(v.x, 1), __shfl_up(v.y, 1)); }
__device__ inline float2 lane_down(const float2 v) { return make_float2(__shfl_down(v.x, 1), __shfl_down(v.y, 1)); }

// the two fluxes of the definition: -((c * (ta + tb)) * (fb - fa))
template <typename R>
__device__ inline R dflux(const R c, const R ta, const R tb, const R fa, const R fb) {
  return -((c * (ta + tb)) * (fb - fa));
}

// Plan layout.  blockIdx.x = tracer * groups + group; a group is 4 / nslice whole tiles (nslice <= 4), wave -> (tile of
// the group, slice).  R2: one 8-byte element (double, or the float2 of two adjacent instances).
template <typename R2>
__global__ void __launch_bounds__(256) wm_diffuse_kernel(const MpdataDiffuseJob b, const long long t0, const int ntile, const int nslice) {
  typedef Elem<R2> E;
  typedef typename E::R R;
  const MpdataLayoutJob& j = b.j;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tpw = 4 / nslice;
  const long long ngrp = ((long long)ntile + tpw - 1) / tpw;
  const int tr = (int)(blockIdx.x / ngrp);
  const long long tl = (blockIdx.x % ngrp) * tpw + wave / nslice;
  const bool wave_on = wave < tpw * nslice && tl < ntile;   // (three slices: the fourth wave idles; the last group may be short)
  const long long tile = t0 + (wave_on ? tl : 0);           // (an idle wave reads tile t0 and stores nothing)
  const int slice = wave % nslice;
  const int nlev = j.nlev, nx = j.ncol_p - 6;
  const int e0 = slice * 64 + lane;
  const bool act = wave_on && e0 < j.chunk;
  const int e = act ? e0 : 0;   // (idle lanes of the last slice read element 0 and store nothing)
  const int s = e / nlev, kk = e - s * nlev;
  const bool has_dn = kk >= 1, has_up = kk + 1 < nlev;   // kk -+ 1 is a level of the same instance
  // the lane's own element, and the neighbour of the wave's first / last lane in the slice next to it
  const bool edge = act && ((lane == 0 && has_dn) || (lane == 63 && has_up));
  const int ee = !edge ? e : (lane == 0 ? e - 1 : e + 1);
  const long long rem_e = j.chunk - j.main_e;
  const bool main_o = e < j.main_e, main_e = ee < j.main_e;
  const long long so = main_o ? j.main_e : rem_e, se = main_e ? j.main_e : rem_e;   // column strides
  const long long oo = main_o ? e : (long long)j.ncol_p * j.main_e + (e - j.main_e);
  const long long oe = main_e ? ee : (long long)j.ncol_p * j.main_e + (ee - j.main_e);
  R2* const fb = static_cast<R2*>(j.prv) + (long long)tr * j.prv_tstride + tile * j.prv_tile_stride;   // column slot 0
  const R2* const tb = static_cast<const R2*>(b.tkh) + tile * j.prv_tile_stride;
  R2* const pf = fb + oo;
  const R2* const pfe = fb + oe;
  const R2* const pt = tb + oo;
  const R2* const pte = tb + oe;

  // per half: the instance the slot stands for, its coefficients
  const long long n = b.sel.n, nslots = b.sel.ncrms;
  const long long kc = tile * b.kc_tile_stride + e;
  const R2 rho2 = static_cast<const R2*>(b.rho)[kc], adz2 = static_cast<const R2*>(b.adz)[kc];
  R cxv[E::N], czv[E::N], czm[E::N], ir[E::N];
  long long bi[E::N];
  bool on[E::N], ph[E::N];
  bool any = false;
#pragma unroll
  for (int h = 0; h < E::N; ++h) {
    const long long q = (tile * j.slp + s) * E::N + h;
    ph[h] = E::N == 2 && (nslots & 1) && q == nslots;   // the phantom half follows the plan's last instance
    const long long sl = ph[h] ? nslots - 1 : q;
    const bool ok = act && sl >= b.sel.sl0 && sl < b.sel.sl0 + n;   // else: padding, the partner of a split pair, a neighbour in the tile
    on[h] = ok;
    any = any || ok;
    bi[h] = ok ? sl - b.sel.sl0 : 0;
    cxv[h] = ok ? static_cast<const R*>(b.cx)[bi[h] + n * kk] : (R)0;
    czv[h] = ok && has_up ? static_cast<const R*>(b.cz)[bi[h] + n * kk] : (R)0;
    czm[h] = ok && has_dn ? static_cast<const R*>(b.cz)[bi[h] + n * (kk - 1)] : (R)0;
    ir[h] = (R)1 / (E::get(rho2, h) * E::get(adz2, h));
  }
  const bool wave_any = __ballot(any) != 0;   // (a slice of a tile whose instances all lie outside the block)
  const bool rd_sb = b.sb != nullptr && kk == 0, rd_st = b.st != nullptr && !has_up;

  // column 0 and column 1: Fx(0), and what the walk carries
  R fxm[E::N], zs[E::N], z0[E::N];
  R2 fc = pf[3 * so], tc = pt[3 * so];
  {
    const R2 f0 = pf[2 * so], tk0 = pt[2 * so];
#pragma unroll
    for (int h = 0; h < E::N; ++h) {
      fxm[h] = dflux<R>(cxv[h], E::get(tk0, h), E::get(tc, h), E::get(f0, h), E::get(fc, h));
      zs[h] = 0;
      z0[h] = 0;
    }
  }
  for (int c = 1; c <= nx; c += NB) {
    // ---- every load of the batch: columns c+1 .. c+NB of the lane's own element (the last one is the look-ahead the
    // next batch stores), the edge neighbours and the boundary fluxes of columns c .. c+NB-1 (indices clamped)
    R2 fn[NB], tn[NB], fe[NB], te[NB];
    R sbv[NB][E::N], stv[NB][E::N];
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const long long cs = min(c + u + 1, nx + 1) + 2;
      fn[u] = pf[cs * so];
      tn[u] = pt[cs * so];
    }
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const long long iu = min(c + u, nx);
      fe[u] = fn[u];
      te[u] = tn[u];
      if (edge) {
        fe[u] = pfe[(iu + 2) * se];
        te[u] = pte[(iu + 2) * se];
      }
#pragma unroll
      for (int h = 0; h < E::N; ++h) {
        sbv[u][h] = rd_sb && on[h] ? static_cast<const R*>(b.sb)[bi[h] + n * (iu - 1)] : (R)0;
        stv[u][h] = rd_st && on[h] ? static_cast<const R*>(b.st)[bi[h] + n * (iu - 1)] : (R)0;
      }
    }
    __syncthreads();   // every wave of the workgroup has loaded what this batch's stores overwrite
    if (wave_any) {
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        if (c + u <= nx) {
          const R2 fcur = u ? fn[u ? u - 1 : 0] : fc, tcur = u ? tn[u ? u - 1 : 0] : tc;
          R2 fd = lane_up(fcur), td = lane_up(tcur), fu = lane_down(fcur), tu = lane_down(tcur);
          if (lane == 0) { fd = fe[u]; td = te[u]; }
          if (lane == 63) { fu = fe[u]; tu = te[u]; }
          R2 out = fcur;
#pragma unroll
          for (int h = 0; h < E::N; ++h) {
            const R f_c = E::get(fcur, h), t_c = E::get(tcur, h);
            const R fx = dflux<R>(cxv[h], t_c, E::get(tn[u], h), f_c, E::get(fn[u], h));
            const R fzu = has_up ? dflux<R>(czv[h], t_c, E::get(tu, h), f_c, E::get(fu, h)) : stv[u][h];
            const R fzd = has_dn ? dflux<R>(czm[h], E::get(td, h), t_c, E::get(fd, h), f_c) : sbv[u][h];
            const R nv = f_c - ((fx - fxm[h]) + (fzu - fzd) * ir[h]);
            fxm[h] = fx;
            zs[h] = zs[h] + fzu;
            z0[h] = z0[h] + fzd;
            if (on[h]) E::at(out, h) = nv;
          }
          if (E::N == 2 && ph[E::N - 1] && on[E::N - 1]) E::at(out, E::N - 1) = E::get(out, 0);
          if (any) pf[(long long)(c + u + 2) * so] = out;
        }
      }
    }
    fc = fn[NB - 1];
    tc = tn[NB - 1];
  }
  if (!b.zflux) return;
  // the lane of level kk owns interface kk + 1 (the top: the sum of st); the lane of the lowest level the surface row too
#pragma unroll
  for (int h = 0; h < E::N; ++h) {
    if (!on[h] || ph[h]) continue;
    R* const z = static_cast<R*>(b.zflux) + bi[h] + n * ((long long)(nlev + 1) * tr);
    z[n * (kk + 1)] = zs[h];
    if (kk == 0) z[0] = z0[h];
  }
}

// Reference layout: element (sl, column i, level k, tracer t) at f + sl + ld * ((i + 2) + (nx + 6) * ((k - 1) + nlev * t)), rho
// and adz at sl + ld * (k - 1), tkh (b, i, k) at b + n * (i + (nx + 2) * (k - 1)).  x: instances of the block, y: rows
// r = (k - 1) + nlev * t.  The new interior goes to out (b, i - 1, r); f is only read.
template <typename R>
__global__ void __launch_bounds__(256) ref_diffuse_kernel(const R* __restrict__ f, const R* __restrict__ rho, const R* __restrict__ adz,
                                                         const long long ld, const long long sl0, const long long n, const int nx,
                                                         const int nlev, const long long rows, const R* __restrict__ tkh,
                                                         const R* __restrict__ cx, const R* __restrict__ cz, const R* __restrict__ sb,
                                                         const R* __restrict__ st, R* __restrict__ zflux, R* __restrict__ out) {
  const long long bi = (long long)blockIdx.x * 256 + threadIdx.x;
  if (bi >= n) return;
  const long long sl = sl0 + bi, lstep = ld * (nx + 6), tstep = n * (nx + 2);
  for (long long r = blockIdx.y; r < rows; r += gridDim.y) {
    const long long t = r / nlev;
    const int kk = (int)(r - t * nlev);
    const bool has_dn = kk >= 1, has_up = kk + 1 < nlev;
    const R* const p = f + sl + ld * (2 + (long long)(nx + 6) * r);   // column 0
    const R* const pt = tkh + bi + tstep * kk;
    const R* const pd = has_dn ? p - lstep : p;
    const R* const pu = has_up ? p + lstep : p;
    const R* const ptd = has_dn ? pt - tstep : pt;
    const R* const ptu = has_up ? pt + tstep : pt;
    const R cxv = cx[bi + n * kk];
    const R czv = has_up ? cz[bi + n * kk] : (R)0, czm = has_dn ? cz[bi + n * (kk - 1)] : (R)0;
    const R ir = (R)1 / (rho[sl + ld * kk] * adz[sl + ld * kk]);
    R fc = p[ld], tc = pt[n];
    R fxm = dflux<R>(cxv, pt[0], tc, p[0], fc);
    R zs = 0, z0 = 0;
    R* const o = out + bi + n * ((long long)nx * r);
    for (int i = 1; i <= nx; ++i) {
      const R fn = p[ld * (i + 1)], tn = pt[n * (i + 1)];
      const R fx = dflux<R>(cxv, tc, tn, fc, fn);
      const R fzu = has_up ? dflux<R>(czv, tc, ptu[n * i], fc, pu[ld * i]) : (st ? st[bi + n * (i - 1)] : (R)0);
      const R fzd = has_dn ? dflux<R>(czm, ptd[n * i], tc, pd[ld * i], fc) : (sb ? sb[bi + n * (i - 1)] : (R)0);
      o[n * (i - 1)] = fc - ((fx - fxm) + (fzu - fzd) * ir);
      fxm = fx;
      zs = zs + fzu;
      z0 = z0 + fzd;
      fc = fn;
      tc = tn;
    }
    if (zflux) {
      R* const z = zflux + bi + n * ((long long)(nlev + 1) * t);
      z[n * (kk + 1)] = zs;
      if (kk == 0) z[0] = z0;
    }
  }
}
// ... and back: the interior columns of f := out
template <typename R>
__global__ void __launch_bounds__(256) ref_diffuse_store_kernel(R* __restrict__ f, const long long ld, const long long sl0, const long long n,
                                                               const int nx, const long long rows, const R* __restrict__ out) {
  const long long bi = (long long)blockIdx.x * 256 + threadIdx.x;
  if (bi >= n) return;
  for (long long r = blockIdx.y; r < rows; r += gridDim.y) {
    R* const p = f + (sl0 + bi) + ld * (3 + (long long)(nx + 6) * r);   // column 1
    const R* const o = out + bi + n * ((long long)nx * r);
    for (int i = 0; i < nx; i += NB) {
      R v[NB];
#pragma unroll
      for (int u = 0; u < NB; ++u) v[u] = o[n * min(i + u, nx - 1)];
#pragma unroll
      for (int u = 0; u < NB; ++u)
        if (i + u < nx) p[ld * (i + u)] = v[u];
    }
  }
}

template <typename R>
hipError_t ref_launch(void* f, const void* rho, const void* adz, long long ld, long long sl0, long long n, int nx, int nlev, long long rows,
                      const void* tkh, const void* cx, const void* cz, const void* sb, const void* st, void* zflux, void* scratch,
                      dim3 grid, hipStream_t stream) {
  hipLaunchKernelGGL((ref_diffuse_kernel<R>), grid, dim3(256), 0, stream, static_cast<const R*>(f), static_cast<const R*>(rho),
                     static_cast<const R*>(adz), ld, sl0, n, nx, nlev, rows, static_cast<const R*>(tkh), static_cast<const R*>(cx),
                     static_cast<const R*>(cz), static_cast<const R*>(sb), static_cast<const R*>(st), static_cast<R*>(zflux),
                     static_cast<R*>(scratch));
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((ref_diffuse_store_kernel<R>), grid, dim3(256), 0, stream, static_cast<R*>(f), ld, sl0, n, nx, rows,
                     static_cast<const R*>(scratch));
  return hipGetLastError();
}

}  // namespace

hipError_t mpdata_diffuse_wm(const MpdataDiffuseJob& b, hipStream_t stream) {
  WmGrid g;
  const MpdataLayoutJob& j = b.j;
  if (!b.tkh || !b.rho || !b.adz || !b.cx || !b.cz || b.sel.W != 1 || j.prv_col0 != 0 || j.ncols != j.ncol_p || b.kc_tile_stride < j.chunk)
    return hipErrorInvalidValue;
  const hipError_t e = wm_block_grid(j, b.sel, j.ntr, &g);
  if (e != hipSuccess) return e;
  if (g.nslice > 4) return hipErrorInvalidValue;   // (a tile is a workgroup's at most: 256 elements of a chunk)
  const int tpw = 4 / g.nslice;
  const long long ngrp = ((long long)g.ntile + tpw - 1) / tpw;
  if (ngrp > 2147483647LL / j.ntr) return hipErrorInvalidValue;
  hipLaunchKernelGGL(b.sel.ipe == 1 ? wm_diffuse_kernel<double> : wm_diffuse_kernel<float2>, dim3((unsigned)(ngrp * j.ntr)), dim3(256), 0,
                     stream, b, g.t0, g.ntile, g.nslice);
  return hipGetLastError();
}

hipError_t mpdata_diffuse_ref(void* f, const void* rho, const void* adz, int elem_bytes, long long ld, long long sl0, long long n,
                              int nx, int nlev, int ntr, const void* tkh, const void* cx, const void* cz, const void* sb,
                              const void* st, void* zflux, void* scratch, hipStream_t stream) {
  if (!f || !rho || !adz || !tkh || !cx || !cz || !scratch || ld < 1 || sl0 < 0 || n < 1 || sl0 + n > ld || nx < 1 || nlev < 1 ||
      ntr < 1 || (elem_bytes != 4 && elem_bytes != 8))
    return hipErrorInvalidValue;
  const long long rows = (long long)nlev * ntr;
  dim3 grid;
  if (ref_block_grid(n, rows, &grid) != hipSuccess) return hipErrorInvalidValue;
  return ref_real(elem_bytes, [&](auto r) {
    return ref_launch<decltype(r)>(f, rho, adz, ld, sl0, n, nx, nlev, rows, tkh, cx, cz, sb, st, zflux, scratch, grid, stream);
  });
}
