// mpdata_subside.hip -- large-scale vertical advection of f, in place (include/mpdata_hip.h 3m, mpdata_subside.h): the
// first-order upwind step along k by one velocity per level that a host model applies to every tracer (SAM's
// subsidence), a Jacobi update of EVERY column slot from the OLD field with two coefficients per instance and level.
// The simplest vertical stencil: radius 1 in k, no coupling in x.  A kernel of its own outside the run: nothing is
// fused into the plan kernels, nothing is kept between calls.
//   plan layout: a wave per 64-element slice of a tile's column chunk, lane -> element e = s * nlev + kk, walks all
//     nx + 6 column slots as linear streams, NB columns in flight, cb(k) and cc(k) of every half in registers; f is read
//     once and written once.  f(i,k+-1) are elements e +- 1 of the same column slot: inside a wave they come by a
//     shuffle of the values just loaded, selected only while kk +- 1 stays inside the instance (else the lane's own
//     value: an exact zero difference); lane 0 and lane 63 load theirs from the slice next door.  The update is in place:
//       chunk <= 64 (nz <= 64, windows): a tile's chunk is one wave's, so no other wave reads what this one stores, and
//         a wave issues every load of a column batch before the batch's first store, in program order;
//       above: an instance is 2 .. 4 slices, so a WORKGROUP OWNS WHOLE TILES and per batch every load -- the batch's
//         columns and the edge neighbours of the same columns -- is issued before a __syncthreads(), every store after
//         it.  Columns do not couple, so the loads of the next batch touch nothing this batch stores: the barrier a wave
//         passes before it stores batch b is passed by every wave after its loads of batch b.  Every wave takes part in
//         every barrier; nothing returns early.
//   reference layout: one thread per instance and (level, tracer) row, coalesced along sl.  dsum is a sum over i in
//     rising order, so a thread marches a row; rows k +- 1 then belong to threads of other workgroups, so the new rows
//     go to a scratch array and a second kernel on the same stream copies them into f: the kernel boundary is the order.
// Built with -ffp-contract=off: every operation of the definition is rounded once, in its association.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "mpdata_subside.h"

namespace {

using namespace wm_walk;

__device__ inline double lane_up(const double v) { return __shfl_up(v, 1); }      // the value of lane - 1
__device__ inline double lane_down(const double v) { return __shfl_down(v, 1); }  // the value of lane + 1
__device__ inline float2 lane_up(const float2 v) { return make_float2(__shfl_up(v.x, 1), __shfl_up(v.y, 1)); }
__device__ inline float2 lane_down(const float2 v) { return make_float2(__shfl_down(v.x, 1), __shfl_down(v.y, 1)); }

// the decrement of the definition: two differences, two products, their sum
template <typename R>
__device__ inline R decrement(const R cb, const R cc, const R fd, const R fc, const R fu) {
  const R a = fc - fd, c = fu - fc;
  const R pa = cb * a, pc = cc * c;
  return pa + pc;
}

// Plan layout.  blockIdx.x = tracer * groups + group; a group is 4 / nslice whole tiles (nslice <= 4), wave -> (tile of
// the group, slice).  R2: one 8-byte element (double, or the float2 of two adjacent instances).
template <typename R2>
__global__ void __launch_bounds__(256) wm_subside_kernel(const MpdataSubsideJob b, const long long t0, const int ntile, const int nslice) {
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
  const int nlev = j.nlev, ncol = j.ncol_p;
  const int e0 = slice * 64 + lane;
  const bool act = wave_on && e0 < j.chunk;
  const int e = act ? e0 : 0;   // (idle lanes of the last slice read element 0 and store nothing)
  const int s = e / nlev, kk = e - s * nlev;
  const bool has_dn = kk >= 1, has_up = kk + 1 < nlev;   // kk -+ 1 is a level of the same slot
  // the lane's own element, and the neighbour of the wave's first / last lane in the slice next to it
  const bool edge = act && ((lane == 0 && has_dn) || (lane == 63 && has_up));
  const int ee = !edge ? e : (lane == 0 ? e - 1 : e + 1);
  const long long rem_e = j.chunk - j.main_e;
  const bool main_o = e < j.main_e, main_e = ee < j.main_e;
  const long long so = main_o ? j.main_e : rem_e, se = main_e ? j.main_e : rem_e;   // column strides
  R2* const fb = static_cast<R2*>(j.prv) + (long long)tr * j.prv_tstride + tile * j.prv_tile_stride;   // column slot 0
  R2* const pf = fb + (main_o ? e : (long long)j.ncol_p * j.main_e + (e - j.main_e));
  const R2* const pfe = fb + (main_e ? ee : (long long)j.ncol_p * j.main_e + (ee - j.main_e));

  // per half: the instance and the tall level the slot stands for, its coefficients
  const int nlev_d = b.sel.nz - 1;
  const long long n = b.sel.n, nslots = b.sel.ncrms * b.sel.W;   // slots that are an instance (a window of one)
  R cbv[E::N], ccv[E::N];
  long long di[E::N];   // index of (instance, tall level) in cb, cc and a tracer of dsum
  bool on[E::N], ph[E::N];
  bool any = false;
#pragma unroll
  for (int h = 0; h < E::N; ++h) {
    long long q = (tile * j.slp + s) * E::N + h;
    ph[h] = E::N == 2 && (nslots & 1) && q == nslots;   // the phantom half follows the plan's last slot
    if (ph[h]) q = nslots - 1;
    long long sl = q;
    int k = kk;
    bool ok = act;
    if (b.sel.W > 1) {   // only the levels the window owns
      sl = q / b.sel.W;
      int k0 = 0, nz_w, own0 = 0, own1 = 0;
      ok = ok && mpd_level_window(b.sel.nz, (int)(q - sl * b.sel.W), &k0, &nz_w, &own0, &own1) == b.sel.W;
      k = k0 + kk;
      ok = ok && k + 1 >= own0 && k + 1 <= own1;
    }
    ok = ok && sl >= b.sel.sl0 && sl < b.sel.sl0 + n && k < nlev_d;   // else: padding, the partner of a split pair, a neighbour in the tile
    on[h] = ok;
    any = any || ok;
    di[h] = ok ? (sl - b.sel.sl0) + n * k : 0;
    cbv[h] = ok ? static_cast<const R*>(b.cb)[di[h]] : (R)0;
    ccv[h] = ok ? static_cast<const R*>(b.cc)[di[h]] : (R)0;
  }
  const bool wave_any = __ballot(any) != 0;   // (a slice of a tile whose slots all lie outside the block)
  const bool sync = nslice > 1;               // (one slice: the chunk is this wave's alone)

  R ds[E::N];
#pragma unroll
  for (int h = 0; h < E::N; ++h) ds[h] = 0;
  for (int c = 0; c < ncol; c += NB) {
    // ---- every load of the batch: columns c .. c+NB-1 of the lane's own element and of the edge neighbour (indices
    // clamped, not predicated: the clamped duplicates of the last column are loaded before it is stored and are stored
    // nowhere)
    R2 v[NB], fe[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) v[u] = pf[(long long)min(c + u, ncol - 1) * so];
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      fe[u] = v[u];
      if (edge) fe[u] = pfe[(long long)min(c + u, ncol - 1) * se];
    }
    if (sync) __syncthreads();   // every wave of the workgroup has loaded what this batch's stores overwrite
    if (wave_any) {
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        if (c + u < ncol) {
          const R2 fcur = v[u];
          R2 fd = lane_up(fcur), fu = lane_down(fcur);
          if (lane == 0) fd = fe[u];
          if (lane == 63) fu = fe[u];
          if (!has_dn) fd = fcur;   // clamped: the level itself
          if (!has_up) fu = fcur;
          const bool inner = c + u >= 3 && c + u <= ncol - 4;   // column i = 1 .. nx at slot i + 2
          R2 out = fcur;
#pragma unroll
          for (int h = 0; h < E::N; ++h) {
            const R f_c = E::get(fcur, h);
            const R dec = decrement<R>(cbv[h], ccv[h], E::get(fd, h), f_c, E::get(fu, h));
            const R nv = f_c - dec;
            if (inner) ds[h] = ds[h] + dec;
            if (on[h]) E::at(out, h) = nv;
          }
          if (E::N == 2 && ph[E::N - 1] && on[E::N - 1]) E::at(out, E::N - 1) = E::get(out, 0);
          if (any) pf[(long long)(c + u) * so] = out;
        }
      }
    }
  }
  if (!b.dsum) return;
#pragma unroll
  for (int h = 0; h < E::N; ++h) {
    if (!on[h] || ph[h]) continue;
    static_cast<R*>(b.dsum)[di[h] + n * ((long long)nlev_d * tr)] = ds[h];
  }
}

// Reference layout: element (sl, column slot c, row r = level + nlev * tracer) at f + sl + ld * (c + (nx + 6) * r), cb, cc
// (b, level) at b + n * level, dsum (b, r) at b + n * r.  x: instances of the block, y: rows.  The new row goes to out
// (b, c, r); f is only read.
template <typename R>
__global__ void __launch_bounds__(256) ref_subside_kernel(const R* __restrict__ f, const long long ld, const long long sl0, const long long n,
                                                         const int nx, const int nlev, const long long rows, const R* __restrict__ cb,
                                                         const R* __restrict__ cc, R* __restrict__ dsum, R* __restrict__ out) {
  const long long bi = (long long)blockIdx.x * 256 + threadIdx.x;
  if (bi >= n) return;
  const int ncol = nx + 6;
  const long long lstep = ld * ncol;
  for (long long r = blockIdx.y; r < rows; r += gridDim.y) {
    const int kk = (int)(r % nlev);
    const R* const p = f + (sl0 + bi) + lstep * r;
    const R* const pd = kk >= 1 ? p - lstep : p;   // clamped: the level itself
    const R* const pu = kk + 1 < nlev ? p + lstep : p;
    const R cbv = cb[bi + n * kk], ccv = cc[bi + n * kk];
    R* const o = out + bi + n * ((long long)ncol * r);
    R ds = 0;
    for (int c = 0; c < ncol; ++c) {
      const R f_c = p[ld * c];
      const R dec = decrement<R>(cbv, ccv, pd[ld * c], f_c, pu[ld * c]);
      o[n * c] = f_c - dec;
      if (c >= 3 && c <= ncol - 4) ds = ds + dec;
    }
    if (dsum) dsum[bi + n * r] = ds;
  }
}
// ... and back: every column slot of f := out
template <typename R>
__global__ void __launch_bounds__(256) ref_subside_store_kernel(R* __restrict__ f, const long long ld, const long long sl0, const long long n,
                                                               const int nx, const long long rows, const R* __restrict__ out) {
  const long long bi = (long long)blockIdx.x * 256 + threadIdx.x;
  if (bi >= n) return;
  const int ncol = nx + 6;
  for (long long r = blockIdx.y; r < rows; r += gridDim.y) {
    R* const p = f + (sl0 + bi) + ld * ((long long)ncol * r);
    const R* const o = out + bi + n * ((long long)ncol * r);
    for (int c = 0; c < ncol; c += NB) {
      R v[NB];
#pragma unroll
      for (int u = 0; u < NB; ++u) v[u] = o[n * min(c + u, ncol - 1)];
#pragma unroll
      for (int u = 0; u < NB; ++u)
        if (c + u < ncol) p[ld * (c + u)] = v[u];
    }
  }
}

template <typename R>
hipError_t ref_launch(void* f, long long ld, long long sl0, long long n, int nx, int nlev, long long rows, const void* cb, const void* cc,
                      void* dsum, void* scratch, dim3 grid, hipStream_t stream) {
  hipLaunchKernelGGL((ref_subside_kernel<R>), grid, dim3(256), 0, stream, static_cast<const R*>(f), ld, sl0, n, nx, nlev, rows,
                     static_cast<const R*>(cb), static_cast<const R*>(cc), static_cast<R*>(dsum), static_cast<R*>(scratch));
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((ref_subside_store_kernel<R>), grid, dim3(256), 0, stream, static_cast<R*>(f), ld, sl0, n, nx, rows,
                     static_cast<const R*>(scratch));
  return hipGetLastError();
}

}  // namespace

hipError_t mpdata_subside_wm(const MpdataSubsideJob& b, hipStream_t stream) {
  WmGrid g;
  const MpdataLayoutJob& j = b.j;
  if (!b.cb || !b.cc || j.prv_col0 != 0 || j.ncols != j.ncol_p) return hipErrorInvalidValue;
  const hipError_t e = wm_block_grid(j, b.sel, j.ntr, &g);
  if (e != hipSuccess) return e;
  if (g.nslice > 4) return hipErrorInvalidValue;   // (a tile is a workgroup's at most: 256 elements of a chunk)
  const int tpw = 4 / g.nslice;
  const long long ngrp = ((long long)g.ntile + tpw - 1) / tpw;
  if (ngrp > 2147483647LL / j.ntr) return hipErrorInvalidValue;
  hipLaunchKernelGGL(b.sel.ipe == 1 ? wm_subside_kernel<double> : wm_subside_kernel<float2>, dim3((unsigned)(ngrp * j.ntr)), dim3(256), 0,
                     stream, b, g.t0, g.ntile, g.nslice);
  return hipGetLastError();
}

hipError_t mpdata_subside_ref(void* f, int elem_bytes, long long ld, long long sl0, long long n, int nx, int nlev, int ntr,
                              const void* cb, const void* cc, void* dsum, void* scratch, hipStream_t stream) {
  if (!f || !cb || !cc || !scratch || ld < 1 || sl0 < 0 || n < 1 || sl0 + n > ld || nx < 1 || nlev < 1 || ntr < 1 ||
      (elem_bytes != 4 && elem_bytes != 8))
    return hipErrorInvalidValue;
  const long long rows = (long long)nlev * ntr;
  dim3 grid;
  if (ref_block_grid(n, rows, &grid) != hipSuccess) return hipErrorInvalidValue;
  return ref_real(elem_bytes, [&](auto r) { return ref_launch<decltype(r)>(f, ld, sl0, n, nx, nlev, rows, cb, cc, dsum, scratch, grid, stream); });
}
