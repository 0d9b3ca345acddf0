// mpdata_vsolve.hip -- implicit vertical solve of f, in place (include/mpdata_hip.h 3o, mpdata_vsolve.h): a tridiagonal
// system along k per instance, interior column and tracer, the coefficients shared by the columns and tracers of an
// instance.  The first block call whose recurrence runs along the LEVELS, the lane axis of the plan layout, AND writes
// f.  Kernels of their own outside the run: nothing is fused into the plan kernels, nothing is kept between calls.
//   factors: a small kernel in front forms p = 1 / pivot and g = up * p once per call, one thread per instance,
//     sequential in k -- the divides stay out of the hot kernel, and every column batch takes the same bits.
//   plan layout: the geometry of mpdata_column_path.hip.  A workgroup takes UG adjacent units (8-byte elements of the
//     instance axis) and CB columns: its four waves copy the column slots of the group's tiles as linear streams (lane ->
//     element of the chunk, NB columns in flight) into LDS, re-laid as [column][unit][level] with an odd level stride,
//     together with lo, p, g of the group's units; after a barrier a lane per (unit, column) runs the forward sweep in
//     LDS in place (y over f), then the backward sweep (x over y); after a second barrier the waves store LDS back to f
//     as the same linear streams.  Race freedom: workgroups own disjoint (group, column batch) element sets, nothing
//     couples columns or instances; inside a workgroup every global load of a stage precedes a barrier and every global
//     store follows the sweeps' barrier; idle lanes clamp their addresses and store nothing, and no barrier sits under
//     a condition that differs inside a workgroup.
//     A windowed plan: the workgroup walks the windows of its units upward -- stages a window, continues the forward
//     sweep with y(k-1) carried in the lane's registers, stores y into the owned levels -- and then downward: re-stages
//     what it wrote (each thread reloads the very elements it stored), continues the backward sweep with x(k+1)
//     carried, stores x.  The halves of an fp32 element are then different windows, of one instance or of two, so the
//     halves are swept one after the other in the order of their slots.
//   reference layout: one thread per instance, coalesced along sl, rows (column, tracer) over grid.y; the thread owns
//     its column, so y and then x go into f in place.
// Built with -ffp-contract=off and IEEE divides: every operation of the definition is rounded once, in its association.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "mpdata_vsolve.h"

namespace {

using namespace wm_walk;

// (LDS_ELEMS, the LDS of a workgroup at most, and the column groups of the launch: mpdata_wm_walk.h)

// The workgroups of the plan-layout kernel.  A UNIT is one 8-byte element of the instance axis (an instance, or the pair
// 2 * ue, 2 * ue + 1 of an fp32 plan): slot ue % slp of tile ue / slp, or, in a windowed plan, the tiles ue * W ..
// ue * W + W - 1.  A workgroup takes UG adjacent units (a multiple of slp) and CB adjacent columns.
// The kernel takes what it reads of the job and the geometry in one compact argument (tile and unit indices fit an int:
// a plan has an int of tiles): fewer scalar registers than the job.
struct VsArgs {
  void* f;                    // the plan side of f, first tracer of the call
  const void *lo, *pg;        // pg: p, and g behind its n * (nz - 1) reals
  long long n, sl0, ncrms;
  long long tstride, tile_stride;
  int t0, t1;                 // tiles the block touches
  int g0, ngroup;             // first group, groups
  int chunk, main_e, ncol_p, nlev, slp;
  int W, nz;
  int UG, CB, ncb, ns;        // ns: level stride in LDS (odd)
  int ush;                    // UG = 1 << ush
};

// One sweep of a lane over the levels [l0, l1) of its column in LDS, HN halves of the element in lockstep from half h0:
//   forward  (UP):   m = a(k) * c;  r = v(k) - m;  c = r * b(k);  v(k) = c       a = lo, b = p, c = y(k-1) carried
//   backward (!UP):  m = a(k) * c;  c = v(k) - m;                 v(k) = c       a = g,         c = x(k+1) carried
// NB levels of operands are read ahead of the chain.  on[j]: the half is written (else it keeps what was staged).
template <typename R2, int HN, bool UP>
__device__ inline void sweep(R2* const v, const R2* const a, const R2* const b, const int h0, const int l0, const int l1,
                             typename Elem<R2>::R (&c)[HN], const bool (&on)[HN]) {
  typedef Elem<R2> E;
  typedef typename E::R R;
  constexpr int N = E::N;
  R* const vr = reinterpret_cast<R*>(v);
  for (int kb = 0; kb < l1 - l0; kb += NB) {
    R2 fv[NB], av[NB], bv[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const int ku = min(kb + u, l1 - l0 - 1);
      const int kc = UP ? l0 + ku : l1 - 1 - ku;
      fv[u] = v[kc];
      av[u] = a[kc];
      if (UP) bv[u] = b[kc];
    }
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      if (kb + u < l1 - l0) {
        const int kc = UP ? l0 + kb + u : l1 - 1 - kb - u;
#pragma unroll
        for (int jj = 0; jj < HN; ++jj) {
          const int h = HN == N ? jj : h0;
          const R m = E::get(av[u], h) * c[jj];
          const R r = E::get(fv[u], h) - m;
          c[jj] = UP ? r * E::get(bv[u], h) : r;
          if (on[jj]) vr[kc * N + h] = c[jj];
        }
      }
    }
  }
}

// A uniform value held in vector registers: the windowed kernels have more uniform values than scalar registers.
template <bool V>
__device__ inline long long in_vgpr(long long x) {
  if (V) asm volatile("" : "+v"(x));
  return x;
}

// Plan layout.  blockIdx.x = (tracer * ngroup + group) * ncb + column batch; R2: one 8-byte element (double, or the float2
// of two adjacent slots); WIN: a windowed plan (W > 1, one slot per tile).
template <typename R2, bool WIN>
__global__ void __launch_bounds__(256) wm_vsolve_kernel(const VsArgs g) {
  typedef Elem<R2> E;
  typedef typename E::R R;
  constexpr int N = E::N;
  extern __shared__ __align__(8) unsigned char vs_lds[];
  const int tid0 = threadIdx.x;
  int bx = blockIdx.x;
  const int cb = bx % g.ncb;
  bx /= g.ncb;
  const int gi = bx % g.ngroup;
  const int tr = bx / g.ngroup;
  const int nlev = g.nlev, nx = g.ncol_p - 6, slp = WIN ? 1 : g.slp, W = WIN ? g.W : 1, ns = g.ns, UG = g.UG;
  const int nzm = g.nz - 1;
  const long long n = in_vgpr<WIN>(g.n), sl0 = in_vgpr<WIN>(g.sl0), tile_stride = in_vgpr<WIN>(g.tile_stride);
  const int c0 = cb * g.CB, cbn = min(g.CB, nx - c0);
  const int ue0 = (g.g0 + gi) * UG;
  const int tile0 = WIN ? ue0 : ue0 / slp;
  const int ntg = WIN ? UG : UG / slp;
  const int nslice = WIN ? 1 : (g.chunk + 63) / 64;   // (a window is 63 levels at most)
  const int rem_e = g.chunk - g.main_e;
  R2* const lf = reinterpret_cast<R2*>(vs_lds);   // [column][unit][ns]: f, then y, then x
  R2* const ll = lf + g.CB * UG * ns;             // [unit][ns]: lo
  R2* const lp = ll + UG * ns;                    //             p
  R2* const lg = lp + UG * ns;                    //             g
  R2* const f = static_cast<R2*>(g.f) + (long long)tr * g.tstride;
  const R* const glo = static_cast<const R*>(g.lo);
  const R* const gp = static_cast<const R*>(g.pg);
  const long long goff = in_vgpr<WIN>(g.n * nzm);   // g lies behind p
  R carry[N];   // per instance of the unit: y(k-1) on the way up, x(k+1) on the way down
  // a windowed plan: the constants of the windows the halves of the W tiles of a unit are, once, through LDS (read back
  // per lane: held by the scalar unit, the window arithmetic and its 64-bit divide spill scalar registers)
  int* const lwin = reinterpret_cast<int*>(lg + UG * ns);   // [tile of the unit][half]{k0, first owned, last owned + 1, instance of the unit}
  if (WIN) {
    const int tid = tid0;
    if (tid < W * N) {
      int k0 = 0, nz_w, own0 = 1, own1 = 0;
      if (mpd_level_window(g.nz, tid % W, &k0, &nz_w, &own0, &own1) != W) own1 = own0 - 1;
      lwin[4 * tid] = k0; lwin[4 * tid + 1] = own0 - 1 - k0; lwin[4 * tid + 2] = max(own1 - k0, own0 - 1 - k0); lwin[4 * tid + 3] = tid / W;
    }
    __syncthreads();
  }

  for (int pass = 0; pass < (WIN ? 2 : 1); ++pass) {
#pragma unroll
    for (int a = 0; a < N; ++a) carry[a] = 0;
    for (int mi = 0; mi < W; ++mi) {
      const int m = pass ? W - 1 - mi : mi;
      // the thread's places are formed anew per window: what the compiler could hoist out of this loop -- a dozen lane
      // conditions, two scalar registers each -- is more than the scalar unit has to spare
      int tid = tid0;
      if (WIN) asm volatile("" : "+v"(tid));
      const int lane = tid & 63, wave = tid >> 6;
      const int ci = tid >> g.ush, ug = tid & (UG - 1);   // the lane's pair in the sweeps
      const bool act = ci < cbn;
      const int ue = ue0 + ug;
      if (pass || mi) __syncthreads();   // the stores of the window before are through with LDS
      // per half of tile (unit, m): slot q = (unit * W + m) * N + h is window q % W of instance unit * N + dih; its owned
      // levels are [l0h, l1h) of the chunk, level kk of it the tall level k0h + kk (a plain plan: all of them, k0h = 0)
      int k0h[N], l0h[N], l1h[N], dih[N];
#pragma unroll
      for (int h = 0; h < N; ++h) {
        k0h[h] = 0; l0h[h] = 0; l1h[h] = nlev; dih[h] = h;
        if (WIN) {
          const int* const wc = lwin + 4 * (m * N + h);
          k0h[h] = wc[0]; l0h[h] = wc[1]; l1h[h] = wc[2]; dih[h] = wc[3];
        }
      }
      // ---- stage (store = false) or store back (store = true): a wave per tile of the group, lane -> element of the
      // chunk.  An element goes through LDS when one of its halves is a slot of the block (of a window: an owned level).
      auto copy = [&](const bool store) {
        for (int tg = wave; tg < ntg; tg += 4) {
          const int tile = (tile0 + tg) * W + m;
          if (tile < g.t0 || tile > g.t1) continue;
          int lo = 0, hi = g.chunk;
          if (WIN) {
            lo = nlev; hi = 0;
#pragma unroll
            for (int h = 0; h < N; ++h) {
              const long long sl = (long long)(tile0 + tg) * N + dih[h];
              if (sl >= sl0 && sl < sl0 + n && l1h[h] > l0h[h]) { lo = min(lo, l0h[h]); hi = max(hi, l1h[h]); }
            }
            if (hi <= lo) continue;
          }
          R2* const src = f + (long long)tile * tile_stride;
          for (int sc = 0; sc < nslice; ++sc) {
            const int e0 = sc * 64 + lane;
            bool in = e0 >= lo && e0 < hi;
            const int e = in ? e0 : lo;   // (idle lanes read an element that is read anyway and store nothing)
            const int es = WIN ? 0 : e / nlev, ek = e - es * nlev;   // (a window: one slot per tile)
            if (!WIN) {
              const long long sa = ((long long)tile * slp + es) * N;
              in = in && sa + N > sl0 && sa < sl0 + n;
            }
            const bool in_main = e < g.main_e;
            const long long cstep = in_main ? g.main_e : rem_e;
            R2* const p = src + (in_main ? e : (long long)g.ncol_p * g.main_e + (e - g.main_e)) + (3 + c0) * cstep;   // column 1 = slot 3
            R2* const d = lf + (long long)(tg * slp + es) * ns + ek;
            for (int i = 0; i < cbn; i += NB) {
              if (!store) {
                R2 v[NB];
#pragma unroll
                for (int u = 0; u < NB; ++u) v[u] = p[(long long)min(i + u, cbn - 1) * cstep];
#pragma unroll
                for (int u = 0; u < NB; ++u)
                  if (in && i + u < cbn) d[(long long)(i + u) * UG * ns] = v[u];
              } else {
                R2 v[NB];
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
      // the coefficients of the group's units by tall level, the unit fastest: adjacent lanes read adjacent instances.
      // A half outside the block takes +0; lo of tall level 1 is not read (+0), g of the top level is +0 as written.
      for (int x = tid; x < UG * nlev; x += 256) {
        const int kk = x >> g.ush, u2 = x & (UG - 1);
        R2 a2, p2, g2;
#pragma unroll
        for (int h = 0; h < N; ++h) {
          const long long sl = (long long)(ue0 + u2) * N + dih[h];
          const int kt = k0h[h] + kk;
          R av = 0, pv = 0, gv = 0;
          if (sl >= sl0 && sl < sl0 + n && kt < nzm) {
            const long long o = (sl - sl0) + n * kt;
            if (kt > 0) av = glo[o];
            pv = gp[o];
            gv = gp[o + goff];
          }
          E::at(a2, h) = av; E::at(p2, h) = pv; E::at(g2, h) = gv;
        }
        ll[u2 * ns + kk] = a2; lp[u2 * ns + kk] = p2; lg[u2 * ns + kk] = g2;
      }
      __syncthreads();
      // ---- the sweeps: a lane per (unit, column)
      if (act) {
        R2* const pf = lf + ((long long)ci * UG + ug) * ns;
        const R2* const pa = ll + ug * ns;
        const R2* const pp = lp + ug * ns;
        const R2* const pg = lg + ug * ns;
        if (!WIN) {
          bool on[N], any = false;
#pragma unroll
          for (int h = 0; h < N; ++h) {
            const long long sl = (long long)ue * N + h;
            on[h] = sl >= sl0 && sl < sl0 + n;
            any = any || on[h];
          }
          if (any) {
            sweep<R2, N, true>(pf, pa, pp, 0, 0, nlev, carry, on);
#pragma unroll
            for (int a = 0; a < N; ++a) carry[a] = 0;
            sweep<R2, N, false>(pf, pg, pg, 0, 0, nlev, carry, on);
            // the phantom half follows the plan's last instance, its partner in the pair
            if (N == 2 && (g.ncrms & 1) && (long long)ue * N + 1 == g.ncrms && on[0]) {
              for (int k = 0; k < nlev; ++k) {
                R2 v = pf[k];
                E::at(v, N - 1) = E::get(v, 0);
                pf[k] = v;
              }
            }
          }
        } else {
          const int tile = ue * W + m;
#pragma unroll
          for (int hh = 0; hh < N; ++hh) {
            const int h = pass ? N - 1 - hh : hh;   // downward: the higher slot first
            const int di1 = h ? dih[N - 1] : dih[0], l0 = h ? l0h[N - 1] : l0h[0], l1 = h ? l1h[N - 1] : l1h[0];   // (selects, no indexing)
            const long long sl = (long long)ue * N + di1;
            const bool on1[1] = {tile >= g.t0 && tile <= g.t1 && sl >= sl0 && sl < sl0 + n && l1 > l0};
            if (on1[0]) {
              R c1[1] = {di1 ? carry[N - 1] : carry[0]};
              if (pass == 0) sweep<R2, 1, true>(pf, pa, pp, h, l0, l1, c1, on1);
              else sweep<R2, 1, false>(pf, pg, pg, h, l0, l1, c1, on1);
              if (di1) carry[N - 1] = c1[0]; else carry[0] = c1[0];
            }
          }
        }
      }
      __syncthreads();
      copy(true);
    }
  }
}

// The factors.  lo, di, up, p, g (n, nlev), leading dimension n.
template <typename R>
__global__ void __launch_bounds__(256) vsolve_factor_kernel(const R* __restrict__ lo, const R* __restrict__ di, const R* __restrict__ up,
                                                           const long long n, const int nlev, R* __restrict__ p, R* __restrict__ g) {
  const long long bi = (long long)blockIdx.x * 256 + threadIdx.x;
  if (bi >= n) return;
  R gk = 0;
  for (int k = 0; k < nlev; ++k) {
    const long long o = bi + n * k;
    R d = di[o];
    if (k > 0) {
      const R m = lo[o] * gk;
      d = d - m;
    }
    const R pk = (R)1 / d;
    gk = 0;
    if (k + 1 < nlev) gk = up[o] * pk;
    p[o] = pk;
    g[o] = gk;
  }
}

// Reference layout: element (sl, column i, level k, tracer t) at f + sl + ld * ((i + 2) + (nx + 6) * ((k - 1) + nlev * t)).
// x: instances of the block, y: rows r = (i - 1) + nx * t.
template <typename R>
__global__ void __launch_bounds__(256) ref_vsolve_kernel(R* f, const R* __restrict__ lo, const R* __restrict__ p, const R* __restrict__ g,
                                                        const long long ld, const long long sl0, const long long n, const int nx,
                                                        const int nlev, const long long rows) {
  const long long bi = (long long)blockIdx.x * 256 + threadIdx.x;
  if (bi >= n) return;
  const long long sl = sl0 + bi, step = ld * (nx + 6);
  for (long long r = blockIdx.y; r < rows; r += gridDim.y) {
    const long long t = r / nx, i = r - t * nx;
    R* const q = f + sl + ld * ((i + 3) + (long long)(nx + 6) * nlev * t);
    R c = 0;
    for (int k = 0; k < nlev; k += NB) {
      R v[NB], a[NB], b[NB];
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        const long long kc = min(k + u, nlev - 1);
        v[u] = q[kc * step];
        a[u] = kc > 0 ? lo[bi + n * kc] : (R)0;
        b[u] = p[bi + n * kc];
      }
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        if (k + u < nlev) {
          const R m = a[u] * c;
          const R rr = v[u] - m;
          c = rr * b[u];
          q[(long long)(k + u) * step] = c;
        }
      }
    }
    c = 0;
    for (int k = 0; k < nlev; k += NB) {
      R v[NB], a[NB];
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        const long long kc = nlev - 1 - min(k + u, nlev - 1);
        v[u] = q[kc * step];
        a[u] = g[bi + n * kc];
      }
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        if (k + u < nlev) {
          const R m = a[u] * c;
          c = v[u] - m;
          q[(long long)(nlev - 1 - k - u) * step] = c;
        }
      }
    }
  }
}

}  // namespace

hipError_t mpdata_vsolve_factor(const void* lo, const void* di, const void* up, int elem_bytes, long long n, int nlev, void* p, void* g,
                                hipStream_t stream) {
  if (!lo || !di || !up || !p || !g || n < 1 || nlev < 1 || (elem_bytes != 4 && elem_bytes != 8)) return hipErrorInvalidValue;
  dim3 grid;
  if (ref_block_grid(n, 1, &grid) != hipSuccess) return hipErrorInvalidValue;
  return ref_real(elem_bytes, [&](auto r) {
    typedef decltype(r) R;
    hipLaunchKernelGGL((vsolve_factor_kernel<R>), grid, dim3(256), 0, stream, static_cast<const R*>(lo), static_cast<const R*>(di),
                       static_cast<const R*>(up), n, nlev, static_cast<R*>(p), static_cast<R*>(g));
    return hipGetLastError();
  });
}

hipError_t mpdata_vsolve_wm(const MpdataVsolveJob& b, hipStream_t stream) {
  WmGrid wg;
  const MpdataLayoutJob& j = b.j;
  if (!b.lo || !b.pg || j.prv_col0 != 0 || j.ncols != j.ncol_p) return hipErrorInvalidValue;
  const hipError_t e = wm_block_grid(j, b.sel, j.ntr, &wg);
  if (e != hipSuccess) return e;
  const int slp = j.slp, W = b.sel.W;
  VsArgs g;
  g.f = j.prv; g.lo = b.lo; g.pg = b.pg;
  g.n = b.sel.n; g.sl0 = b.sel.sl0; g.ncrms = b.sel.ncrms;
  g.tstride = j.prv_tstride; g.tile_stride = j.prv_tile_stride;
  g.t0 = (int)wg.t0; g.t1 = (int)(wg.t0 + wg.ntile - 1);
  g.chunk = (int)j.chunk; g.main_e = (int)j.main_e; g.ncol_p = j.ncol_p; g.nlev = j.nlev; g.slp = slp;
  g.W = W; g.nz = b.sel.nz;
  if (W > 128 || (W > 1 && j.chunk > 64)) return hipErrorInvalidValue;   // (the window table: a thread per slot of a unit; nz < 7000)
  const int win_e = W > 1 ? 2 * W * b.sel.ipe : 0;   // the window table: 16 bytes per slot of a unit
  // the three coefficient rows next to the columns; the kernel forms the tiles of a windowed plan from units, in int
  ColGroups cg;
  if (j.chunk > 2147483647LL || j.main_e > 2147483647LL ||
      !col_groups_batched(j, b.sel, wg, LDS_ELEMS, /*fixed*/ win_e, /*rows*/ 3, /*unit_mul*/ W, &cg))
    return hipErrorInvalidValue;
  col_groups_fill(cg, &g);
  g.ncb = cg.ncb; g.ush = cg.ush;
  const unsigned blocks = (unsigned)(cg.ngroup * j.ntr * g.ncb);
  const size_t lds = (size_t)cg.lds_e * 8;
  void (*k)(VsArgs) = b.sel.ipe == 1 ? (W > 1 ? wm_vsolve_kernel<double, true> : wm_vsolve_kernel<double, false>)
                                     : (W > 1 ? wm_vsolve_kernel<float2, true> : wm_vsolve_kernel<float2, false>);
  hipLaunchKernelGGL(k, dim3(blocks), dim3(256), lds, stream, g);
  return hipGetLastError();
}

hipError_t mpdata_vsolve_ref(void* f, int elem_bytes, long long ld, long long sl0, long long n, int nx, int nlev, int ntr, const void* lo,
                             const void* p, const void* g, hipStream_t stream) {
  if (!f || !lo || !p || !g || ld < 1 || sl0 < 0 || n < 1 || sl0 + n > ld || nx < 1 || nlev < 1 || ntr < 1 ||
      (elem_bytes != 4 && elem_bytes != 8))
    return hipErrorInvalidValue;
  const long long rows = (long long)nx * ntr;
  dim3 grid;
  if (ref_block_grid(n, rows, &grid) != hipSuccess) return hipErrorInvalidValue;
  return ref_real(elem_bytes, [&](auto r) {
    typedef decltype(r) R;
    hipLaunchKernelGGL((ref_vsolve_kernel<R>), grid, dim3(256), 0, stream, static_cast<R*>(f), static_cast<const R*>(lo),
                       static_cast<const R*>(p), static_cast<const R*>(g), ld, sl0, n, nx, nlev, rows);
    return hipGetLastError();
  });
}
