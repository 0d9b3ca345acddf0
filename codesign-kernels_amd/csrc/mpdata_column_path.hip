// mpdata_column_path.hip -- mass-weighted column integrals of f per instance, interior column and tracer, and their sum
// over the columns (include/mpdata_hip.h 3k, mpdata_column_path.h): the one block call that reduces along the LEVELS, the
// lane axis of the plan layout, in a kernel of its own outside the run (nothing is fused into the plan kernels, nothing
// is kept between calls).
//   plan layout: the sum is sequential in k, so a lane owns one (slot, column) pair and walks its levels.  Read where they
//     lie, those are 8 bytes per lane and 128-byte line, so a workgroup stages them through LDS instead: its four waves
//     copy the column slots of a group of adjacent tiles as the linear streams the other block kernels read (lane ->
//     element of the chunk, NB columns in flight), re-laid as [column][slot][level] with an odd level stride, together
//     with the products rho * adz of the group's slots; then every lane sums its column from LDS, NB reads in flight.
//     A group holds 16 adjacent 8-byte elements of the instance axis, so a store of path is a whole 128-byte line.
//     The windows of a tall plan are staged one after the other, the running sums stay in the lanes' registers.
//   reference layout: one thread per instance, coalesced along sl, the loop over k inside.
// Built with -ffp-contract=off: every operation of the definition is rounded once, in the definition's association.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "mpdata_column_path.h"

namespace {

using namespace wm_walk;

constexpr int CP_LDS_ELEMS = 4096;   // 8-byte elements of LDS per workgroup (32 KiB: five workgroups per CU)

// The workgroups of the plan-layout kernel: column groups (mpdata_wm_walk.h: units, groups of UG units, batches of CB
// columns) as col_groups_batched makes them; the tiles, the first group and the number of groups in long long -- the
// kernel counts units in long long.
struct CpGeom {
  long long t0, t1;   // tiles the block touches
  long long g0;       // first group
  long long ngroup;
  int UG, CB, ncb, ns;   // ns: level stride in LDS (odd)
};

// the levels [lo, hi) of its chunk slot that slot q adds to instance *sl: all of them, of a window the owned ones; none
// for padding, the phantom, the partner of a split pair and neighbours in the tile
__device__ inline void slot_levels(const MpdataBlockSel& sel, const int nlev, const long long q, long long* sl, int* lo, int* hi) {
  *sl = q; *lo = 0; *hi = nlev;
  if (sel.W > 1) {
    *sl = q / sel.W;
    int k0 = 0, nz_w, own0 = 1, own1 = 0;
    if (mpd_level_window(sel.nz, (int)(q - *sl * sel.W), &k0, &nz_w, &own0, &own1) != sel.W) own1 = own0 - 1;
    *lo = own0 - 1 - k0;
    *hi = own1 - k0;
  }
  if (*sl < sel.sl0 || *sl >= sel.sl0 + sel.n || *hi < *lo) *hi = *lo = 0;
}

// Plan layout.  blockIdx.x = (tracer * ngroup + group) * ncb + column batch; R2: one 8-byte element.
template <typename R2>
__global__ void __launch_bounds__(256) wm_column_path_kernel(const MpdataColumnPathJob b, const CpGeom g) {
  typedef Elem<R2> E;
  typedef typename E::R R;
  extern __shared__ __align__(8) unsigned char cp_lds[];
  const MpdataLayoutJob& j = b.j;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  long long bx = blockIdx.x;
  const int cb = (int)(bx % g.ncb);
  bx /= g.ncb;
  const long long gi = bx % g.ngroup;
  const int tr = (int)(bx / g.ngroup);
  const int nlev = j.nlev, nx = j.ncol_p - 6, slp = j.slp, W = b.sel.W, ns = g.ns, UG = g.UG;
  const int c0 = cb * g.CB, cbn = min(g.CB, nx - c0);
  const long long ue0 = (g.g0 + gi) * UG;
  const long long tile0 = ue0 / slp;   // (W > 1: slp = 1)
  const int ntg = UG / slp;
  const int nslice = (int)((j.chunk + 63) / 64);
  const long long rem_e = j.chunk - j.main_e;
  R2* const lf = reinterpret_cast<R2*>(cp_lds);       // [column][unit][ns]
  R2* const lw = lf + (long long)g.CB * UG * ns;      // [unit][ns]: rho * adz
  const R2* const f = static_cast<const R2*>(j.prv) + (long long)tr * j.prv_tstride;
  // the lane's pair in the sums
  const int ci = tid / UG, ug = tid - ci * UG;
  const bool act = ci < cbn;
  const long long ue = ue0 + ug;
  const int s = (int)(ue % slp);
  R acc[E::N];
#pragma unroll
  for (int a = 0; a < E::N; ++a) acc[a] = 0;

  for (int m = 0; m < W; ++m) {
    if (m) __syncthreads();   // the sums of the window before are through with LDS
    // ---- stage: a wave per tile of the group, lane -> element of the chunk
    for (int tg = wave; tg < ntg; tg += 4) {
      const long long tile = (tile0 + tg) * W + m;
      if (tile < g.t0 || tile > g.t1) continue;
      int lo = 0, hi = (int)j.chunk;
      if (W > 1) {   // the owned levels of the halves that belong to the block
        lo = nlev; hi = 0;
#pragma unroll
        for (int h = 0; h < E::N; ++h) {
          long long sl;
          int l0, l1;
          slot_levels(b.sel, nlev, tile * E::N + h, &sl, &l0, &l1);
          if (l1 > l0) { lo = min(lo, l0); hi = max(hi, l1); }
        }
        if (hi <= lo) continue;
      }
      const R2* const src = f + tile * j.prv_tile_stride;
      for (int sc = 0; sc < nslice; ++sc) {
        const int e0 = sc * 64 + lane;
        const bool in = e0 >= lo && e0 < hi;
        const int e = in ? e0 : lo;   // (idle lanes read an element that is read anyway and store nothing)
        const int es = e / nlev, ek = e - es * nlev;
        const bool in_main = e < j.main_e;
        const long long cstep = in_main ? j.main_e : rem_e;
        const R2* const p = src + (in_main ? e : (long long)j.ncol_p * j.main_e + (e - j.main_e)) + (3 + c0) * cstep;   // column 1 = slot 3
        R2* const d = lf + (long long)(tg * slp + es) * ns + ek;
        for (int i = 0; i < cbn; i += NB) {
          R2 v[NB];
#pragma unroll
          for (int u = 0; u < NB; ++u) v[u] = p[(long long)min(i + u, cbn - 1) * cstep];
#pragma unroll
          for (int u = 0; u < NB; ++u)
            if (in && i + u < cbn) d[(long long)(i + u) * UG * ns] = v[u];
        }
      }
    }
    // the weights of the group's slots, one rounded multiply per level
    for (int x = tid; x < UG * nlev; x += 256) {
      const int u2 = x / nlev, kk = x - u2 * nlev;
      const long long ue2 = ue0 + u2;
      const long long tile = ue2 / slp * W + m;
      if (tile < g.t0 || tile > g.t1) continue;
      const long long o = tile * b.kc_tile_stride + (ue2 % slp) * nlev + kk;
      const R2 r2 = static_cast<const R2*>(b.rho)[o], a2 = static_cast<const R2*>(b.adz)[o];
      R2 w2;
#pragma unroll
      for (int h = 0; h < E::N; ++h) E::at(w2, h) = E::get(r2, h) * E::get(a2, h);
      lw[u2 * ns + kk] = w2;
    }
    __syncthreads();
    // ---- the sums: a lane per (unit, column), its levels in rising order
    if (act) {
      const long long tile = ue / slp * W + m;
      const R2* const pf = lf + ((long long)ci * UG + ug) * ns;
      const R2* const pw = lw + ug * ns;
#pragma unroll
      for (int h = 0; h < E::N; ++h) {
        long long sl;
        int lo, hi;
        slot_levels(b.sel, nlev, (tile * slp + s) * E::N + h, &sl, &lo, &hi);
        if (tile < g.t0 || tile > g.t1) hi = lo;
        const bool first = sl == ue * E::N;   // which of the unit's instances the slot belongs to
        R sum = first ? acc[0] : acc[E::N - 1];
        for (int kk = lo; kk < hi; kk += NB) {
          R2 v[NB], w[NB];
#pragma unroll
          for (int u = 0; u < NB; ++u) {
            const int kc = min(kk + u, hi - 1);
            v[u] = pf[kc];
            w[u] = pw[kc];
          }
#pragma unroll
          for (int u = 0; u < NB; ++u)
            if (kk + u < hi) sum = sum + E::get(w[u], h) * E::get(v[u], h);
        }
        if (first) acc[0] = sum; else acc[E::N - 1] = sum;
      }
    }
  }
  if (!act) return;
#pragma unroll
  for (int a = 0; a < E::N; ++a) {
    const long long sl = ue * E::N + a;
    if (sl < b.sel.sl0 || sl >= b.sel.sl0 + b.sel.n) continue;   // padding, phantom, the partner of a split pair, a neighbour in the group
    static_cast<R*>(b.path)[(sl - b.sel.sl0) + b.sel.n * ((c0 + ci) + (long long)nx * tr)] = acc[a];
  }
}

// Reference layout: element (sl, column i, level k, tracer t) at f + sl + ld * ((i + 2) + (nx + 6) * ((k - 1) + nlev * t)), rho
// and adz at sl + ld * (k - 1).  x: instances of the block, y: rows r = (i - 1) + nx * t.
template <typename R>
__global__ void __launch_bounds__(256) ref_column_path_kernel(const R* f, const R* rho, const R* adz, const long long ld, const long long sl0,
                                                             const long long n, const int nx, const int nlev, const long long rows, R* path) {
  const long long bi = (long long)blockIdx.x * 256 + threadIdx.x;
  if (bi >= n) return;
  const long long sl = sl0 + bi, step = ld * (nx + 6);
  for (long long r = blockIdx.y; r < rows; r += gridDim.y) {
    const long long t = r / nx, i = r - t * nx;
    const R* const p = f + sl + ld * ((i + 3) + (long long)(nx + 6) * nlev * t);
    R sum = 0;
    for (int k = 0; k < nlev; k += NB) {
      R v[NB], rv[NB], av[NB];
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        const long long kc = min(k + u, nlev - 1);
        v[u] = p[kc * step];
        rv[u] = rho[sl + ld * kc];
        av[u] = adz[sl + ld * kc];
      }
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        if (k + u < nlev) {
          const R w = rv[u] * av[u];
          sum = sum + w * v[u];
        }
      }
    }
    path[bi + n * r] = sum;
  }
}

// mass(b, t) = the sequential sum over i of path(b, i, t).  x: instances of the block, y: tracers.
template <typename R>
__global__ void __launch_bounds__(256) column_mass_kernel(const R* path, const long long n, const int nx, const int ntr, R* mass) {
  const long long bi = (long long)blockIdx.x * 256 + threadIdx.x;
  if (bi >= n) return;
  for (long long t = blockIdx.y; t < ntr; t += gridDim.y) {
    const R* const p = path + bi + n * nx * t;
    R sum = 0;
    for (int i = 0; i < nx; i += NB) {
      R v[NB];
#pragma unroll
      for (int u = 0; u < NB; ++u) v[u] = p[n * min(i + u, nx - 1)];
#pragma unroll
      for (int u = 0; u < NB; ++u)
        if (i + u < nx) sum = sum + v[u];
    }
    mass[bi + n * t] = sum;
  }
}

hipError_t column_mass(const void* path, int elem_bytes, long long n, int nx, int ntr, void* mass, hipStream_t stream) {
  dim3 grid, block(256);
  if (ref_block_grid(n, ntr, &grid) != hipSuccess) return hipErrorInvalidValue;
  return ref_real(elem_bytes, [&](auto r) {
    typedef decltype(r) R;
    hipLaunchKernelGGL((column_mass_kernel<R>), grid, block, 0, stream, static_cast<const R*>(path), n, nx, ntr, static_cast<R*>(mass));
    return hipGetLastError();
  });
}

}  // namespace

hipError_t mpdata_column_path_wm(const MpdataColumnPathJob& b, hipStream_t stream) {
  WmGrid wg;
  const MpdataLayoutJob& j = b.j;
  if (!b.rho || !b.adz || !b.path || j.prv_col0 != 0 || j.ncols != j.ncol_p || b.kc_tile_stride < j.chunk) return hipErrorInvalidValue;
  hipError_t e = wm_block_grid(j, b.sel, j.ntr, &wg);
  if (e != hipSuccess) return e;
  // one row of rho * adz next to the columns: 16 units = one 128-byte line of path per column; the kernel counts units
  // in long long
  ColGroups cg;
  if (!col_groups_batched(j, b.sel, wg, CP_LDS_ELEMS, /*fixed*/ 0, /*rows*/ 1, /*unit_mul*/ 0, &cg)) return hipErrorInvalidValue;
  CpGeom g;
  g.t0 = wg.t0; g.t1 = wg.t0 + wg.ntile - 1;
  col_groups_fill(cg, &g);
  g.ncb = cg.ncb;
  const unsigned blocks = (unsigned)(g.ngroup * j.ntr * g.ncb);
  hipLaunchKernelGGL(b.sel.ipe == 1 ? wm_column_path_kernel<double> : wm_column_path_kernel<float2>, dim3(blocks), dim3(256),
                     (size_t)cg.lds_e * 8, stream, b, g);
  e = hipGetLastError();
  if (e != hipSuccess || !b.mass) return e;
  return column_mass(b.path, 8 / b.sel.ipe, b.sel.n, j.ncol_p - 6, j.ntr, b.mass, stream);
}

hipError_t mpdata_column_path_ref(const void* f, const void* rho, const void* adz, int elem_bytes, long long ld, long long sl0,
                                  long long n, int nx, int nlev, int ntr, void* path, void* mass, hipStream_t stream) {
  if (!f || !rho || !adz || !path || ld < 1 || sl0 < 0 || n < 1 || sl0 + n > ld || nx < 1 || nlev < 1 || ntr < 1 ||
      (elem_bytes != 4 && elem_bytes != 8))
    return hipErrorInvalidValue;
  const long long rows = (long long)nx * ntr;
  dim3 grid, block(256);
  if (ref_block_grid(n, rows, &grid) != hipSuccess) return hipErrorInvalidValue;
  const hipError_t e = ref_real(elem_bytes, [&](auto r) {
    typedef decltype(r) R;
    hipLaunchKernelGGL((ref_column_path_kernel<R>), grid, block, 0, stream, static_cast<const R*>(f), static_cast<const R*>(rho),
                       static_cast<const R*>(adz), ld, sl0, n, nx, nlev, rows, static_cast<R*>(path));
    return hipGetLastError();
  });
  if (e != hipSuccess || !mass) return e;
  return column_mass(path, elem_bytes, n, nx, ntr, mass, stream);
}
