// mpdata_vdiffuse.hip -- implicit vertical diffusion of f with a per-cell diffusivity, in place (include/mpdata_hip.h 3s,
// mpdata_vdiffuse.h): backward Euler of 3l's vertical part, a tridiagonal system along k per instance, interior column
// and tracer whose matrix is formed from tkh(i,k) and cz(k) per COLUMN -- the factorisation is per column too, where
// mpdata_vsolve.hip takes it per instance from a kernel in front.  Kernels of their own outside the run: nothing is fused
// into the plan kernels, nothing is kept between calls.
//   1 / (rho * adz): a small kernel in front (the one of mpdata_column_step.hip, restated) forms it once per call, one
//     rounded multiply and one IEEE divide per (instance, level), so that every column takes the same bits.
//   plan layout: the geometry and the copy stage of mpdata_vsolve.hip (plain plans only).  A workgroup takes UG adjacent
//     units (8-byte elements of the instance axis) and CB columns: its four waves copy the column slots of the group's
//     tiles as linear streams (lane -> element of the chunk, NB columns in flight) into LDS, re-laid as
//     [column][unit][level] with an odd level stride; all its threads stage the rows of tkh of those instances and
//     columns beside them in the same arrangement, read where they lie (the unit fastest: 16 fp64 or 32 fp32 adjacent
//     instances are one 128-byte line), and cz and ir of the group's units per (unit, level).  After a barrier a lane per
//     (unit, column) runs the forward sweep in LDS in place -- y over f, and g(k) over tkh(k) once e(k) is formed, so a cell
//     takes two LDS elements, not three -- then the backward sweep (x over y); after a second barrier the waves store
//     LDS back to f as the same linear streams.  One launch covers the tracers of the call, a workgroup per (tracer,
//     group, column batch): the factors are formed again per tracer, as mpdata_vsolve.hip stages its factors again.
//     Race freedom: workgroups own disjoint (tracer, group, column batch) element sets, nothing couples columns or
//     instances; inside a workgroup every global load (f, tkh, cz, ir, sb, st) precedes the first barrier and every global
//     store follows the sweeps' barrier; between them a lane touches only its own column in LDS; idle lanes clamp their
//     addresses and store nothing, and no barrier sits under a condition that differs inside a workgroup.
//     LDS: VD_LDS_ELEMS, one constant; the launch refuses a geometry that exceeds it.
//   reference layout: one thread per instance and column, coalesced along sl, the columns over grid.y, the tracers one
//     after the other inside the thread; the thread owns its columns, so y and then x go into f in place, and g(k) into
//     the caller's scratch array, written and read back by the same thread.
// Built with -ffp-contract=off and IEEE divides: every operation of the definition is rounded once, in its association.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "mpdata_vdiffuse.h"

namespace {

using namespace wm_walk;

// 8-byte elements of LDS per workgroup at most: 2 * (CB + 1) * UG * ns of them are used (f and tkh / g per cell, cz and
// ir per (unit, level)).  The budget of the neighbours (mpdata_wm_walk.h): docs/EXPERIMENTS.md AC has the times of this and
// of the 80 KiB form.
constexpr int VD_LDS_ELEMS = LDS_ELEMS;   // 40 KiB: room for four workgroups per CU
constexpr int LA = 4;   // levels of operands read ahead of the chain

// One level of the forward sweep: ep = e(k-1), ek = e(k), irk = ir(k), r = r(k); gp, yp: g(k-1), y(k-1) in, g(k), y(k) out.
template <typename R>
__device__ inline void forward_level(const bool first, const R ep, const R ek, const R irk, const R r, R& gp, R& yp) {
  const R a = ep * irk;
  const R c = ek * irk;
  const R t = (R)1 + a;
  const R di = t + c;
  R d = di, v = r;
  if (!first) {
    const R m = a * gp;
    d = di - m;
    const R q = a * yp;
    v = r + q;
  }
  const R p = (R)1 / d;
  gp = c * p;
  yp = v * p;
}
// r(k) of level index k (0-based) from f(i,k): the boundary fluxes enter the first and the last level
template <typename R>
__device__ inline R rhs_level(const int k, const int nlev, const R fv, const R irk, const bool hsb, const R sbv, const bool hst, const R stv) {
  R r = fv;
  if (k == 0 && hsb) {
    const R pr = sbv * irk;
    r = r + pr;
  }
  if (k == nlev - 1 && hst) {
    const R pr = stv * irk;
    r = r - pr;
  }
  return r;
}

template <typename R>
struct VdArgs {
  void* f;                    // the plan side of f, first tracer of the call
  const R *tkh, *cz, *ir, *sb, *st;
  long long n, sl0, ncrms;
  long long tstride, tile_stride;
  int t0, t1;                 // tiles the block touches
  int g0, ngroup;             // first group, groups
  int chunk, main_e, ncol_p, nlev, slp;
  int UG, CB, ncb, ns;        // ns: level stride in LDS (odd)
  int ush;                    // UG = 1 << ush
};

// Plan layout.  blockIdx.x = (tracer * ngroup + group) * ncb + column batch; R2: one 8-byte element (double, or the float2
// of two adjacent slots).
template <typename R2>
__global__ void __launch_bounds__(256) wm_vdiffuse_kernel(const VdArgs<typename Elem<R2>::R> g) {
  typedef Elem<R2> E;
  typedef typename E::R R;
  constexpr int N = E::N;
  extern __shared__ __align__(8) unsigned char vd_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int bx = blockIdx.x;
  const int cb = bx % g.ncb;
  bx /= g.ncb;
  const int gi = bx % g.ngroup;
  const int tr = bx / g.ngroup;
  const int nlev = g.nlev, nx = g.ncol_p - 6, slp = g.slp, ns = g.ns, UG = g.UG;
  const long long n = g.n, sl0 = g.sl0;
  const int c0 = cb * g.CB, cbn = min(g.CB, nx - c0);
  const int ue0 = (g.g0 + gi) * UG;
  const int tile0 = ue0 / slp, ntg = UG / slp;
  const int nslice = (g.chunk + 63) / 64;
  const int rem_e = g.chunk - g.main_e;
  R2* const lf = reinterpret_cast<R2*>(vd_lds);   // [column][unit][ns]: f, then y, then x
  R2* const lt = lf + g.CB * UG * ns;             // [column][unit][ns]: tkh, then g
  R2* const lc = lt + g.CB * UG * ns;             // [unit][ns]: cz (+0 at the top level)
  R2* const li = lc + UG * ns;                    //             ir
  R2* const f = static_cast<R2*>(g.f) + (long long)tr * g.tstride;
  const int ci = tid >> g.ush, ug = tid & (UG - 1);   // the lane's pair in the sweeps (dense: dealt to the four waves in
  const bool act = ci < cbn;                          // equal shares the call is 9 % slower, docs/EXPERIMENTS.md AC)
  const int ue = ue0 + ug;

  // ---- stage (store = false) or store back (store = true): a wave per tile of the group, lane -> element of the chunk.
  // An element goes through LDS when one of its halves is a slot of the block.
  auto copy = [&](const bool store) {
    for (int tg = wave; tg < ntg; tg += 4) {
      const int tile = tile0 + tg;
      if (tile < g.t0 || tile > g.t1) continue;
      R2* const src = f + (long long)tile * g.tile_stride;
      for (int sc = 0; sc < nslice; ++sc) {
        const int e0 = sc * 64 + lane;
        bool in = e0 < g.chunk;
        const int e = in ? e0 : 0;   // (idle lanes read an element that is read anyway and store nothing)
        const int es = e / nlev, ek = e - es * nlev;
        const long long sa = ((long long)tile * slp + es) * N;
        in = in && sa + N > sl0 && sa < sl0 + n;
        const bool in_main = e < g.main_e;
        const long long cstep = in_main ? g.main_e : rem_e;
        R2* const p = src + (in_main ? e : (long long)g.ncol_p * g.main_e + (e - g.main_e)) + (3 + c0) * cstep;   // column 1 = slot 3
        R2* const d = lf + (long long)(tg * slp + es) * ns + ek;
        for (int i = 0; i < cbn; i += NB) {
          R2 v[NB];
          if (!store) {
#pragma unroll
            for (int u = 0; u < NB; ++u) v[u] = p[(long long)min(i + u, cbn - 1) * cstep];
#pragma unroll
            for (int u = 0; u < NB; ++u)
              if (in && i + u < cbn) d[(long long)(i + u) * UG * ns] = v[u];
          } else {
#pragma unroll
            for (int u = 0; u < NB; ++u) v[u] = d[(long long)min(i + u, cbn - 1) * UG * ns];
#pragma unroll
            for (int u = 0; u < NB; ++u)
              if (in && i + u < cbn) p[(long long)(i + u) * cstep] = v[u];
          }
        }
      }
    }
  };
  copy(false);
  // ---- tkh of the batch's columns (column c0 + c of the interior is column c0 + c + 1 of tkh's 0:nx+1), cz and ir of the
  // group's units, the unit fastest: adjacent lanes read adjacent instances.  A half outside the block takes +0.
  {
    const long long tl = n * (nx + 2);   // level stride of tkh
    for (int x = tid; x < UG * nlev; x += 256) {
      const int kk = x >> g.ush, u2 = x & (UG - 1);
      long long bi[N];
      bool in[N];
#pragma unroll
      for (int h = 0; h < N; ++h) {
        const long long sl = (long long)(ue0 + u2) * N + h;
        in[h] = sl >= sl0 && sl < sl0 + n;
        bi[h] = in[h] ? sl - sl0 : 0;
      }
      R2 c2, i2;
#pragma unroll
      for (int h = 0; h < N; ++h) {
        R cv = 0, iv = 0;
        if (in[h]) {
          if (kk < nlev - 1) cv = g.cz[bi[h] + n * kk];   // (cz of the top level is never read)
          iv = g.ir[bi[h] + n * kk];
        }
        E::at(c2, h) = cv; E::at(i2, h) = iv;
      }
      lc[u2 * ns + kk] = c2; li[u2 * ns + kk] = i2;
      const R* const tk = g.tkh + n * (c0 + 1) + tl * kk;
      R2* const d = lt + u2 * ns + kk;
      for (int c = 0; c < cbn; c += LA) {
        R2 v[LA];
#pragma unroll
        for (int u = 0; u < LA; ++u) {
          const long long o = n * min(c + u, cbn - 1);
#pragma unroll
          for (int h = 0; h < N; ++h) E::at(v[u], h) = in[h] ? tk[bi[h] + o] : (R)0;
        }
#pragma unroll
        for (int u = 0; u < LA; ++u)
          if (c + u < cbn) d[(long long)(c + u) * UG * ns] = v[u];
      }
    }
  }
  // the lane's boundary fluxes
  bool on[N], any = false;
  R sbv[N], stv[N];
#pragma unroll
  for (int h = 0; h < N; ++h) {
    const long long sl = (long long)ue * N + h;
    on[h] = act && sl >= sl0 && sl < sl0 + n;
    any = any || on[h];
    const long long o = (on[h] ? sl - sl0 : 0) + n * (act ? c0 + ci : 0);
    sbv[h] = g.sb && on[h] ? g.sb[o] : (R)0;
    stv[h] = g.st && on[h] ? g.st[o] : (R)0;
  }
  const bool hsb = g.sb != nullptr, hst = g.st != nullptr;
  __syncthreads();
  // ---- the sweeps: a lane per (unit, column)
  if (any) {
    R2* const pf = lf + ((long long)ci * UG + ug) * ns;
    R2* const pt = lt + ((long long)ci * UG + ug) * ns;
    const R2* const pc = lc + ug * ns;
    const R2* const pi = li + ug * ns;
    R* const fr = reinterpret_cast<R*>(pf);
    R ep[N], gp[N], yp[N];
#pragma unroll
    for (int h = 0; h < N; ++h) { ep[h] = 0; gp[h] = 0; yp[h] = 0; }
    for (int kb = 0; kb < nlev; kb += LA) {
      R2 fv[LA], tv[LA + 1], cv[LA], iv[LA];
#pragma unroll
      for (int u = 0; u < LA; ++u) {
        const int k = min(kb + u, nlev - 1);
        fv[u] = pf[k]; tv[u] = pt[k]; cv[u] = pc[k]; iv[u] = pi[k];
      }
      tv[LA] = pt[min(kb + LA, nlev - 1)];
#pragma unroll
      for (int u = 0; u < LA; ++u) {
        if (kb + u < nlev) {
          const int k = kb + u;
          R2 gv;
#pragma unroll
          for (int h = 0; h < N; ++h) {
            const R s = E::get(tv[u], h) + E::get(tv[u + 1], h);
            R ek = E::get(cv[u], h) * s;
            if (k == nlev - 1) ek = 0;
            const R irk = E::get(iv[u], h);
            const R r = rhs_level<R>(k, nlev, E::get(fv[u], h), irk, hsb, sbv[h], hst, stv[h]);
            forward_level<R>(k == 0, ep[h], ek, irk, r, gp[h], yp[h]);
            ep[h] = ek;
            E::at(gv, h) = gp[h];
            if (on[h]) fr[k * N + h] = yp[h];
          }
          pt[k] = gv;   // (tkh(k + 1) of the next batch is read after this store: it is another element)
        }
      }
    }
    // backward: x(nlev) = y(nlev) is in place; xk carries x(k+1)
    for (int kb = 1; kb < nlev; kb += LA) {
      R2 yv[LA], gv[LA];
#pragma unroll
      for (int u = 0; u < LA; ++u) {
        const int k = nlev - 1 - min(kb + u, nlev - 1);
        yv[u] = pf[k]; gv[u] = pt[k];
      }
#pragma unroll
      for (int u = 0; u < LA; ++u) {
        if (kb + u < nlev) {
          const int k = nlev - 1 - kb - u;
#pragma unroll
          for (int h = 0; h < N; ++h) {
            const R m = E::get(gv[u], h) * yp[h];
            yp[h] = E::get(yv[u], h) + m;
            if (on[h]) fr[k * N + h] = yp[h];
          }
        }
      }
    }
    // the phantom half follows the plan's last instance, its partner in the pair
    if (N == 2 && (g.ncrms & 1) && (long long)ue * N + 1 == g.ncrms && on[0]) {
      for (int k = 0; k < nlev; ++k) {
        R2 v = pf[k];
        E::at(v, N - 1) = E::get(v, 0);
        pf[k] = v;
      }
    }
  }
  __syncthreads();
  copy(true);
}

// 1 / (rho * adz) of the block's instances from the plan's kc array ([tile][rho, adz, rhow][slot][level], 8-byte elements)
// into ir (n, nlev), leading dimension n: one rounded multiply, one IEEE divide.  x: instances of the block, y: levels.
template <typename R2>
__global__ void __launch_bounds__(256) vd_ir_kernel(const R2* __restrict__ rho, const R2* __restrict__ adz, const long long kc_tile_stride,
                                                   const long long sl0, const long long n, const int slp, const int nlev,
                                                   typename Elem<R2>::R* __restrict__ ir) {
  typedef Elem<R2> E;
  typedef typename E::R R;
  constexpr int N = E::N;
  const long long b0 = (long long)blockIdx.x * 256 + threadIdx.x;
  if (b0 >= n) return;
  const long long sl = sl0 + b0, ue = sl / N, tile = ue / slp;
  const int h = (int)(sl - ue * N), slot = (int)(ue - tile * slp);
  for (int k = blockIdx.y; k < nlev; k += gridDim.y) {
    const long long o = tile * kc_tile_stride + slot * nlev + k;
    ir[b0 + n * k] = (R)1 / (E::get(rho[o], h) * E::get(adz[o], h));
  }
}

// Reference layout: element (sl, column i, level k, tracer t) at f + sl + ld * ((i + 2) + (nx + 6) * ((k - 1) + nlev * t)), rho
// and adz at sl + ld * (k - 1).  x: instances of the block, y: columns.
template <typename R>
__global__ void __launch_bounds__(256) ref_vdiffuse_kernel(R* f, const R* __restrict__ rho, const R* __restrict__ adz,
                                                          const R* __restrict__ tkh, const R* __restrict__ cz, const R* __restrict__ sb,
                                                          const R* __restrict__ st, R* gbuf, const long long ld, const long long sl0,
                                                          const long long n, const int nx, const int nlev, const int ntr) {
  const long long b0 = (long long)blockIdx.x * 256 + threadIdx.x;
  if (b0 >= n) return;
  const long long sl = sl0 + b0, step = ld * (nx + 6), tl = n * (nx + 2), gl = n * nx;
  const bool hsb = sb != nullptr, hst = st != nullptr;
  for (long long i = blockIdx.y; i < nx; i += gridDim.y) {
    const R* const tk = tkh + b0 + n * (i + 1);
    R* const gq = gbuf + b0 + n * i;
    const R sbv = hsb ? sb[b0 + n * i] : (R)0, stv = hst ? st[b0 + n * i] : (R)0;
    for (int t = 0; t < ntr; ++t) {
      R* const q = f + sl + ld * ((i + 3) + (long long)(nx + 6) * nlev * t);
      R ep = 0, gp = 0, yp = 0;
      R tc = tk[0];
      for (int k = 0; k < nlev; ++k) {
        R ek = 0, tn = tc;
        if (k < nlev - 1) {
          tn = tk[tl * (k + 1)];
          const R s = tc + tn;
          ek = cz[b0 + n * k] * s;
        }
        const R irk = (R)1 / (rho[sl + ld * k] * adz[sl + ld * k]);
        const R r = rhs_level<R>(k, nlev, q[step * k], irk, hsb, sbv, hst, stv);
        forward_level<R>(k == 0, ep, ek, irk, r, gp, yp);
        ep = ek; tc = tn;
        gq[gl * k] = gp;
        q[step * k] = yp;
      }
      for (int k = nlev - 2; k >= 0; --k) {
        const R m = gq[gl * k] * yp;
        yp = q[step * k] + m;
        q[step * k] = yp;
      }
    }
  }
}

template <typename R2>
hipError_t wm_launch(const MpdataVdiffuseJob& b, const WmGrid& wg, hipStream_t stream) {
  typedef typename Elem<R2>::R R;
  const MpdataLayoutJob& j = b.j;
  VdArgs<R> g;
  g.f = j.prv;
  g.tkh = static_cast<const R*>(b.tkh); g.cz = static_cast<const R*>(b.cz); g.ir = static_cast<const R*>(b.ir);
  g.sb = static_cast<const R*>(b.sb); g.st = static_cast<const R*>(b.st);
  g.n = b.sel.n; g.sl0 = b.sel.sl0; g.ncrms = b.sel.ncrms;
  g.tstride = j.prv_tstride; g.tile_stride = j.prv_tile_stride;
  g.t0 = (int)wg.t0; g.t1 = (int)(wg.t0 + wg.ntile - 1);
  g.chunk = (int)j.chunk; g.main_e = (int)j.main_e; g.ncol_p = j.ncol_p; g.nlev = j.nlev; g.slp = j.slp;
  // two LDS elements per cell and two rows (cz, ir): the geometry of CB columns and ONE row in HALF the budget, doubled
  ColGroups cg;
  if (j.chunk > 2147483647LL || j.main_e > 2147483647LL ||
      !col_groups_batched(j, b.sel, wg, VD_LDS_ELEMS / 2, /*fixed*/ 0, /*rows*/ 1, /*unit_mul*/ 1, &cg))
    return hipErrorInvalidValue;
  cg.lds_e *= 2;
  if (cg.lds_e > VD_LDS_ELEMS) return hipErrorInvalidValue;
  col_groups_fill(cg, &g);
  g.ncb = cg.ncb; g.ush = cg.ush;
  const unsigned blocks = (unsigned)(cg.ngroup * j.ntr * g.ncb);
  const size_t lds = (size_t)cg.lds_e * 8;
  dim3 grid;
  if (ref_block_grid(b.sel.n, j.nlev, &grid) != hipSuccess) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vd_ir_kernel<R2>, grid, dim3(256), 0, stream, static_cast<const R2*>(b.rho), static_cast<const R2*>(b.adz),
                     b.kc_tile_stride, b.sel.sl0, b.sel.n, j.slp, j.nlev, static_cast<R*>(b.ir));
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(wm_vdiffuse_kernel<R2>, dim3(blocks), dim3(256), lds, stream, g);
  return hipGetLastError();
}

}  // namespace

hipError_t mpdata_vdiffuse_wm(const MpdataVdiffuseJob& b, hipStream_t stream) {
  WmGrid wg;
  const MpdataLayoutJob& j = b.j;
  if (!b.tkh || !b.cz || !b.rho || !b.adz || !b.ir || b.sel.W != 1 || j.prv_col0 != 0 || j.ncols != j.ncol_p ||
      b.kc_tile_stride < j.chunk)
    return hipErrorInvalidValue;
  const hipError_t e = wm_block_grid(j, b.sel, j.ntr, &wg);
  if (e != hipSuccess) return e;
  return b.sel.ipe == 1 ? wm_launch<double>(b, wg, stream) : wm_launch<float2>(b, wg, stream);
}

hipError_t mpdata_vdiffuse_ref(void* f, const void* rho, const void* adz, int elem_bytes, long long ld, long long sl0, long long n,
                               int nx, int nlev, int ntr, const void* tkh, const void* cz, const void* sb, const void* st, void* gbuf,
                               hipStream_t stream) {
  if (!f || !rho || !adz || !tkh || !cz || !gbuf || ld < 1 || sl0 < 0 || n < 1 || sl0 + n > ld || nx < 1 || nlev < 1 || ntr < 1 ||
      (elem_bytes != 4 && elem_bytes != 8))
    return hipErrorInvalidValue;
  dim3 grid;
  if (ref_block_grid(n, nx, &grid) != hipSuccess) return hipErrorInvalidValue;
  return ref_real(elem_bytes, [&](auto r) {
    typedef decltype(r) R;
    hipLaunchKernelGGL((ref_vdiffuse_kernel<R>), grid, dim3(256), 0, stream, static_cast<R*>(f), static_cast<const R*>(rho),
                       static_cast<const R*>(adz), static_cast<const R*>(tkh), static_cast<const R*>(cz), static_cast<const R*>(sb),
                       static_cast<const R*>(st), static_cast<R*>(gbuf), ld, sl0, n, nx, nlev, ntr);
    return hipGetLastError();
  });
}
