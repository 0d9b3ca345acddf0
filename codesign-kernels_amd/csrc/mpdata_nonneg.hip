// mpdata_nonneg.hip -- conservative per-level non-negativity fixer of f, in place (include/mpdata_hip.h 3x, mpdata_nonneg.h):
// the negative cells of a level's interior row become +0 and the others are scaled by r = s / p, the row's sum over the sum
// of its positive cells, so that the row keeps its total; a row whose total is not positive becomes +0 throughout, and a
// row without a negative cell is read and not stored.  A kernel of its own outside the run: nothing is fused into the plan
// kernels, nothing is kept between calls.
//   plan layout: the walk of mpdata_wm_walk.h over the column slots 3 .. nx+2, a lane per element.  Two forms: KEPT,
//     nx <= KEPT_NX = 32 -- all columns of the lane's element are loaded into registers, reduced, and by the lanes in need
//     scaled and stored, so f is loaded once --, and RE-READ, every other nx -- a reducing walk, the outputs, and, unless no
//     lane of the wave is in need, the updating walk over the same columns; nothing of f stays in registers between the
//     walks.  Both give the same bits.  A lane touches the columns of its own element only, so there is no LDS, no barrier
//     and no ordering to argue.
//   reference layout: one thread per instance and (level, tracer) row, coalesced along sl, two loops over i; in place.
// Built with -ffp-contract=off and IEEE divides: every operation of the definition is rounded once, in its association.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "mpdata_nonneg.h"

namespace {

using namespace wm_walk;

// one column of the reduction: s = s + x; y = (x > 0) ? x : +0; p = p + y; c = c + ((x < 0) ? 1 : 0)
template <typename R>
__device__ inline void reduce_one(const R x, R& s, R& p, R& c) {
  s = s + x;
  const R y = x > (R)0 ? x : (R)0;
  p = p + y;
  c = c + (x < (R)0 ? (R)1 : (R)0);
}
// the factor of a row in need: s / p where the row has mass left, else +0 (y * +0 = +0 for every y >= +0)
template <typename R>
__device__ inline R row_factor(const R s, const R p) {
  const R q = s / p;
  return s > (R)0 ? q : (R)0;
}
// one column of the update
template <typename R>
__device__ inline R fix_one(const R x, const R r) {
  const R y = x > (R)0 ? x : (R)0;
  return y * r;
}

// s, p and c of the nx values q[0], q[step], ... of every lane: all NB loads of a batch are issued before the first is used
// (the index is clamped, not predicated); the batch's tail is cut by wave-uniform conditions.
template <typename R2>
__device__ inline void march_reduce(const R2* q, const long long step, const int nx, typename Elem<R2>::R (&s)[Elem<R2>::N],
                                    typename Elem<R2>::R (&p)[Elem<R2>::N], typename Elem<R2>::R (&c)[Elem<R2>::N]) {
  typedef Elem<R2> E;
#pragma unroll
  for (int h = 0; h < E::N; ++h) s[h] = p[h] = c[h] = 0;
  for (int i = 0; i < nx; i += NB) {
    R2 v[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) v[u] = q[(long long)min(i + u, nx - 1) * step];
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      if (i + u < nx) {
#pragma unroll
        for (int h = 0; h < E::N; ++h) reduce_one(E::get(v[u], h), s[h], p[h], c[h]);
      }
    }
  }
}

// nx elements q[0], q[step], ... of a lane := y * r: all NB loads of a batch are issued before the first store (clamped
// duplicates of the last column are loaded before that column is stored and are stored nowhere).  A half with on[h] false
// keeps the bits it was loaded with; follow: the second half takes the first half's result (the phantom); a lane with no
// half on stores nothing.
template <typename R2>
__device__ inline void march_fix(R2* q, const long long step, const int nx, const typename Elem<R2>::R (&r)[Elem<R2>::N],
                                 const bool (&on)[Elem<R2>::N], const bool follow) {
  typedef Elem<R2> E;
  typedef typename E::R R;
  bool any = false;
#pragma unroll
  for (int h = 0; h < E::N; ++h) any = any || on[h];
  for (int i = 0; i < nx; i += NB) {
    R2 v[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) v[u] = q[(long long)min(i + u, nx - 1) * step];
    if (any) {
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        if (i + u < nx) {
#pragma unroll
          for (int h = 0; h < E::N; ++h) {
            R& x = E::at(v[u], h);
            const R z = fix_one(x, r[h]);
            x = on[h] ? z : x;
          }
          if (E::N == 2 && follow) E::at(v[u], E::N - 1) = E::get(v[u], 0);
          q[(long long)(i + u) * step] = v[u];
        }
      }
    }
  }
}

// The KEPT form, nx <= KEPT_NX: the columns of the lane's element stay in registers between the reduction and the update,
// so f is loaded once.  Fully unrolled and statically indexed (no scratch); the loads go out in groups of NB with the index
// clamped inside a group, the groups cut by wave-uniform conditions.  Reduction, factor and update are those of
// march_reduce and march_fix, in the same order: the same bits.  in[h]: the half is a row of the block; followable: the
// second half is the phantom of the plan's last slot.
constexpr int KEPT_NX = 32;
template <typename R2>
__device__ inline void march_kept(R2* q, const long long step, const int nx, const bool (&in)[Elem<R2>::N], const bool followable,
                                  typename Elem<R2>::R* const (&ps)[Elem<R2>::N], typename Elem<R2>::R* const (&pn)[Elem<R2>::N]) {
  typedef Elem<R2> E;
  typedef typename E::R R;
  R2 v[KEPT_NX];
#pragma unroll
  for (int g = 0; g < KEPT_NX; g += NB) {
    if (g < nx) {
#pragma unroll
      for (int u = 0; u < NB; ++u) v[g + u] = q[(long long)min(g + u, nx - 1) * step];
    }
  }
  R s[E::N], p[E::N], c[E::N];
#pragma unroll
  for (int h = 0; h < E::N; ++h) s[h] = p[h] = c[h] = 0;
#pragma unroll
  for (int i = 0; i < KEPT_NX; ++i) {
    if (i < nx) {
#pragma unroll
      for (int h = 0; h < E::N; ++h) reduce_one(E::get(v[i], h), s[h], p[h], c[h]);
    }
  }
  bool on[E::N], any = false;
#pragma unroll
  for (int h = 0; h < E::N; ++h) {
    if (ps[h]) *ps[h] = s[h];
    if (pn[h]) *pn[h] = c[h];
    on[h] = in[h] && c[h] > (R)0;
    any = any || on[h];
  }
  if (!any) return;
  R r[E::N];
#pragma unroll
  for (int h = 0; h < E::N; ++h) r[h] = row_factor(s[h], p[h]);
  const bool follow = followable && on[0];
#pragma unroll
  for (int i = 0; i < KEPT_NX; ++i) {
    if (i < nx) {
#pragma unroll
      for (int h = 0; h < E::N; ++h) {
        R& x = E::at(v[i], h);
        const R z = fix_one(x, r[h]);
        x = on[h] ? z : x;
      }
      if (E::N == 2 && follow) E::at(v[i], E::N - 1) = E::get(v[i], 0);
      q[(long long)i * step] = v[i];
    }
  }
}

// Plan layout: a wave per (tracer, tile of the block, 64-element slice of the chunk), lane -> element e = s * nlev + kk.
// R2: one 8-byte element (double, or the float2 of two adjacent slots); KEPT (nx <= KEPT_NX): march_kept in the place of
// the two marches.
template <typename R2, bool KEPT>
__device__ inline void wm_nonneg(const MpdataNonnegJob& b, const long long t0, const int ntile, const int nslice) {
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
  R2* q = static_cast<R2*>(j.prv) + (long long)tr * j.prv_tstride + tile * j.prv_tile_stride +
          (in_main ? e : (long long)j.ncol_p * j.main_e + (e - j.main_e)) + 3 * cstep;   // column 1 = slot 3
  // per half: the instance and the tall level the slot stands for and its place in sum and nneg
  const int nzm = b.sel.nz - 1;
  const long long nslots = b.sel.ncrms * b.sel.W;   // slots that are an instance (a window of one)
  bool in[E::N], any_in = false;
  long long o[E::N];
#pragma unroll
  for (int h = 0; h < E::N; ++h) {
    const long long slot = (tile * j.slp + s) * E::N + h;
    long long sl = slot;
    int k = kk;
    bool ok = act;
    if (b.sel.W > 1) {
      sl = slot / b.sel.W;
      int k0 = 0, nz_w, own0 = 1, own1 = 0;
      ok = ok && mpd_level_window(b.sel.nz, (int)(slot - sl * b.sel.W), &k0, &nz_w, &own0, &own1) == b.sel.W;
      k = k0 + kk;
      ok = ok && k + 1 >= own0 && k + 1 <= own1;   // the level's owner alone reads and writes it
    }
    // else: padding, the phantom, the partner of a split pair, a neighbour in the tile
    ok = ok && sl >= b.sel.sl0 && sl < b.sel.sl0 + b.sel.n && k < nzm;
    in[h] = ok;
    any_in = any_in || ok;
    o[h] = (ok ? (sl - b.sel.sl0) + b.sel.n * (long long)k : 0) + b.sel.n * ((long long)nzm * tr);
  }
  if (__ballot(any_in) == 0) return;   // (a slice whose elements all lie outside the block: nothing to load)
  // the phantom half of an odd fp32 plan follows the plan's last slot, its partner in the element (W > 1: the caller
  // restores the inner plan's phantom behind the kernel)
  const bool followable = E::N == 2 && b.sel.W == 1 && (nslots & 1) && act && (tile * j.slp + s) * E::N + 1 == nslots;
  if (KEPT) {
    R *ps[E::N], *pn[E::N];
#pragma unroll
    for (int h = 0; h < E::N; ++h) {
      ps[h] = (b.sum && in[h]) ? static_cast<R*>(b.sum) + o[h] : nullptr;
      pn[h] = (b.nneg && in[h]) ? static_cast<R*>(b.nneg) + o[h] : nullptr;
    }
    march_kept<R2>(q, cstep, nx, in, followable, ps, pn);
    return;
  }
  R sm[E::N], p[E::N], c[E::N], r[E::N];
  march_reduce<R2>(q, cstep, nx, sm, p, c);
  bool on[E::N], any = false;
#pragma unroll
  for (int h = 0; h < E::N; ++h) {
    if (b.sum && in[h]) static_cast<R*>(b.sum)[o[h]] = sm[h];
    if (b.nneg && in[h]) static_cast<R*>(b.nneg)[o[h]] = c[h];
    on[h] = in[h] && c[h] > (R)0;
    any = any || on[h];
  }
  if (__ballot(any) == 0) return;   // no row of the wave holds a negative cell: the field is read and not stored
#pragma unroll
  for (int h = 0; h < E::N; ++h) r[h] = row_factor(sm[h], p[h]);
  march_fix<R2>(q, cstep, nx, r, on, followable && on[0]);
}
template <typename R2>
__global__ void __launch_bounds__(256) wm_nonneg_reread_kernel(const MpdataNonnegJob b, const long long t0, const int ntile, const int nslice) {
  wm_nonneg<R2, false>(b, t0, ntile, nslice);
}
// (five waves per SIMD, the occupancy of mpdata_relax.hip's kept form: 96 registers in fp64 where the allocator takes 101
// unasked, no spill)
template <typename R2>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5))) wm_nonneg_kept_kernel(const MpdataNonnegJob b, const long long t0, const int ntile, const int nslice) {
  wm_nonneg<R2, true>(b, t0, ntile, nslice);
}

// Reference layout: element (sl, column i, row r = level + nlev * tracer) at f + sl + ld * ((i + 2) + (nx + 6) * r); sum and
// nneg at bi + n * r.  x: instances of the block, y: rows.
template <typename R>
__global__ void __launch_bounds__(256) ref_nonneg_kernel(R* f, const long long ld, const long long sl0, const long long n, const int nx,
                                                        const long long rows, R* sum, R* nneg) {
  const long long bi = (long long)blockIdx.x * 256 + threadIdx.x;
  if (bi >= n) return;
  for (long long row = blockIdx.y; row < rows; row += gridDim.y) {
    R* const q = f + (sl0 + bi) + ld * ((long long)(nx + 6) * row + 3);   // column 1
    R s[1], p[1], c[1];
    march_reduce<R>(q, ld, nx, s, p, c);
    if (sum) sum[bi + n * row] = s[0];
    if (nneg) nneg[bi + n * row] = c[0];
    const bool on[1] = {c[0] > (R)0};
    if (!on[0]) continue;
    const R r[1] = {row_factor(s[0], p[0])};
    march_fix<R>(q, ld, nx, r, on, false);
  }
}

}  // namespace

hipError_t mpdata_nonneg_wm(const MpdataNonnegJob& b, hipStream_t stream) {
  WmGrid g;
  const hipError_t e = wm_block_grid(b.j, b.sel, b.j.ntr, &g);
  if (e != hipSuccess) return e;
  if (b.j.ncol_p - 6 <= KEPT_NX)   // the columns fit the registers: f is loaded once
    return wm_block_launch(wm_nonneg_kept_kernel<double>, wm_nonneg_kept_kernel<float2>, b, g, stream);
  return wm_block_launch(wm_nonneg_reread_kernel<double>, wm_nonneg_reread_kernel<float2>, b, g, stream);
}

hipError_t mpdata_nonneg_ref(void* f, int elem_bytes, long long ld, long long sl0, long long n, int nx, int nlev, int ntr, void* sum,
                             void* nneg, hipStream_t stream) {
  if (!f || ld < 1 || sl0 < 0 || n < 1 || sl0 + n > ld || nx < 1 || nlev < 1 || ntr < 1) return hipErrorInvalidValue;
  const long long rows = (long long)nlev * ntr;
  dim3 grid, block(256);
  if (ref_block_grid(n, rows, &grid) != hipSuccess) return hipErrorInvalidValue;
  return ref_real(elem_bytes, [&](auto r) {
    typedef decltype(r) R;
    hipLaunchKernelGGL((ref_nonneg_kernel<R>), grid, block, 0, stream, static_cast<R*>(f), ld, sl0, n, nx, rows, static_cast<R*>(sum),
                       static_cast<R*>(nneg));
    return hipGetLastError();
  });
}
