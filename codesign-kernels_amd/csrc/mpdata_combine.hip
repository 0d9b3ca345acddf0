// mpdata_combine.hip -- linear combinations of the tracers of f, in place (include/mpdata_hip.h 3z, mpdata_combine.h):
// f(dst) = sum over j of coef_j * f(src_j) + c0 on the interior columns, optionally clipped at zero, with the level sums of
// the new row -- buoyancy from level profiles, total water, a snapshot and a tendency, a profile written into a tracer, any
// a * x + b * y between tracers.  The first block call that sees a LIST of tracers of a cell.  A kernel of its own outside
// the run: nothing is fused into the plan kernels, nothing is kept between calls.
//   plan layout: the walk of mpdata_wm_walk.h over the column slots 3 .. nx+2, a lane per element, as 1 + nsrc streams --
//     the dst tracer and, at signed 64-bit offsets from it, the sources --, templated on the number of sources, the
//     columns in flight chosen per class; coef and c0 in registers, sum lane-local in column order.  A lane touches the
//     columns of its own element only and loads every source of a batch before the batch's first store, so there is no
//     LDS, no barrier and no ordering to argue, also where dst is a source.
//   reference layout: one thread per instance and level row, coalesced along sl, one loop over i; in place.
// Built with -ffp-contract=off: every operation of the definition is rounded once, in its association; the clip is
// compare-and-select (NaN and -0 fall to the +0 branch), never fmax / fmin.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>

#include "mpdata_combine.h"

namespace {

using namespace wm_walk;

constexpr int NSMAX = MPDATA_COMBINE_NSRC;

// the columns in flight of a kernel with NS sources and `halves` reals per element
constexpr int nb_of(const int NS, const int halves) {
  return NS <= 2 ? MPDATA_COMBINE_NB_LO : NS <= 4 ? MPDATA_COMBINE_NB_MID : MPDATA_COMBINE_HI_SERIAL ? MPDATA_COMBINE_NB_SERIAL
         : halves == 1 ? MPDATA_COMBINE_NB_HI_F64 : MPDATA_COMBINE_NB_HI;
}
constexpr bool serial_of(const int NS) { return NS > 4 && MPDATA_COMBINE_HI_SERIAL != 0; }

// the coefficients of one half of a lane's element (cf[0] alone exists for NS == 0)
template <typename R, int NS>
struct Coef {
  R cf[NS > 0 ? NS : 1];
  R c0;
};

// the offsets of the sources from dst, by value (kernel arguments: scalar registers)
struct Offs {
  long long o[NSMAX];
};

// source j of one cell into the running value: the first is taken (times its coefficient), the others are added
template <typename R, int NS>
__device__ inline void combine_term(R& v, const R x, const Coef<R, NS>& c, const int j, const bool hascoef) {
  const R p = hascoef ? c.cf[j] * x : x;
  v = j == 0 ? p : v + p;
}
// ... and what follows the sources (NS == 0: v = c0)
template <typename R, int NS>
__device__ inline R combine_tail(R v, const Coef<R, NS>& c, const bool hasc0, const bool clip) {
  if (NS == 0) v = c.c0;
  else if (hasc0) v = v + c.c0;
  if (clip) v = (v > (R)0) ? v : (R)0;
  return v;
}

// nx elements p[0], p[step], ... (tracer dst) and p[off.o[j]], p[off.o[j] + step], ... (source j) of a lane: all loads of
// a batch of NBC columns are issued before its first store (clamped duplicates of the last column are loaded before that
// column is stored and are stored nowhere), so a source that is dst is read old.  A half with on[h] false keeps the bits
// dst holds -- keep: the lane loads the dst stream for them, which no other lane does -- and adds nothing to s; follow:
// the second half takes the first half's result (the phantom); a lane with no half on stores nothing.  s[h]: s = +0;
// s = s + v(i), i ascending.
// SERIAL: the sources are walked inside the batch, v[u] accumulated source by source, the loads of source j + 1 issued in
// front of the adds of source j; the adds of a cell are in the order j = 0, 1, ... in both forms.
template <typename R2, int NS, int NBC, bool SERIAL>
__device__ inline void march_combine(R2* p, const Offs& off, const long long step, const int nx,
                                     const Coef<typename Elem<R2>::R, NS> (&c)[Elem<R2>::N], const bool hascoef, const bool hasc0,
                                     const bool clip, const bool (&on)[Elem<R2>::N], const bool follow, const bool keep,
                                     typename Elem<R2>::R (&s)[Elem<R2>::N]) {
  typedef Elem<R2> E;
  typedef typename E::R R;
  bool any = false;
#pragma unroll
  for (int h = 0; h < E::N; ++h) {
    any = any || on[h];
    s[h] = 0;
  }
  for (int i = 0; i < nx; i += NBC) {
    R2 v[NBC], old[NBC];
    if (SERIAL) {
      R2 xa[NBC], xb[NBC];
#pragma unroll
      for (int u = 0; u < NBC; ++u) xa[u] = p[off.o[0] + (long long)min(i + u, nx - 1) * step];
#pragma unroll
      for (int j = 0; j < NS; ++j) {
        if (j + 1 < NS) {
#pragma unroll
          for (int u = 0; u < NBC; ++u) xb[u] = p[off.o[j + 1 < NS ? j + 1 : 0] + (long long)min(i + u, nx - 1) * step];
        }
#pragma unroll
        for (int u = 0; u < NBC; ++u) {
#pragma unroll
          for (int h = 0; h < E::N; ++h) combine_term<R, NS>(E::at(v[u], h), E::get(xa[u], h), c[h], j, hascoef);
          xa[u] = xb[u];
        }
      }
    } else {
      R2 x[NS > 0 ? NS : 1][NBC];
#pragma unroll
      for (int j = 0; j < NS; ++j) {
#pragma unroll
        for (int u = 0; u < NBC; ++u) x[j][u] = p[off.o[j] + (long long)min(i + u, nx - 1) * step];
      }
#pragma unroll
      for (int u = 0; u < NBC; ++u) {
#pragma unroll
        for (int j = 0; j < NS; ++j) {
#pragma unroll
          for (int h = 0; h < E::N; ++h) combine_term<R, NS>(E::at(v[u], h), E::get(x[j][u], h), c[h], j, hascoef);
        }
      }
    }
    if (E::N == 2 && keep) {
#pragma unroll
      for (int u = 0; u < NBC; ++u) old[u] = p[(long long)min(i + u, nx - 1) * step];
    }
    if (any) {
#pragma unroll
      for (int u = 0; u < NBC; ++u) {
        if (i + u < nx) {
#pragma unroll
          for (int h = 0; h < E::N; ++h) {
            const R r = combine_tail<R, NS>(NS > 0 ? E::get(v[u], h) : (R)0, c[h], hasc0, clip);
            if (on[h]) s[h] = s[h] + r;
            E::at(v[u], h) = (on[h] || E::N == 1) ? r : E::get(old[u], h);
          }
          if (E::N == 2 && follow) E::at(v[u], E::N - 1) = E::get(v[u], 0);
          p[(long long)(i + u) * step] = v[u];
        }
      }
    }
  }
}

// Plan layout: a wave per (tile of the block, 64-element slice of the chunk), lane -> element e = s * nlev + kk.
// R2: one 8-byte element (double, or the float2 of two adjacent slots).  NS: the sources.  (256, 4): four waves per
// SIMD, 128 VGPRs at most.
template <typename R2, int NS>
__global__ void __launch_bounds__(256, 4) wm_combine_kernel(const MpdataCombineJob b, const long long t0, const int ntile, const int nslice) {
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
  R2* p = static_cast<R2*>(j.prv) + (long long)b.dst * j.prv_tstride + tile * j.prv_tile_stride +
          (in_main ? e : (long long)j.ncol_p * j.main_e + (e - j.main_e)) + 3 * cstep;   // column 1 = slot 3, tracer dst
  Offs off;
#pragma unroll
  for (int q = 0; q < NSMAX; ++q) off.o[q] = b.off[q];   // signed: a source below dst walks back
  // per half: the instance and the tall level the slot stands for, its coefficients and its place in sum
  const int nzm = b.sel.nz - 1;
  const long long nslots = b.sel.ncrms * b.sel.W;   // slots that are an instance (a window of one)
  const long long cstride = b.sel.n * (long long)nzm;
  Coef<R, NS> c[E::N];
  bool on[E::N];
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
    on[h] = ok;
    o[h] = ok ? (sl - b.sel.sl0) + b.sel.n * (long long)k : 0;
#pragma unroll
    for (int q2 = 0; q2 < (NS > 0 ? NS : 1); ++q2)
      c[h].cf[q2] = (b.coef && ok && NS > 0) ? static_cast<const R*>(b.coef)[o[h] + cstride * q2] : (R)1;
    c[h].c0 = (b.c0 && ok) ? static_cast<const R*>(b.c0)[o[h]] : (R)0;
  }
  // the phantom half of an odd fp32 plan follows the plan's last slot, its partner in the element (W > 1: the caller
  // restores the inner plan's phantom behind the kernel)
  const bool follow = E::N == 2 && b.sel.W == 1 && (nslots & 1) && act && (tile * j.slp + s) * E::N + 1 == nslots && on[0];
  bool any = false, all = true;
#pragma unroll
  for (int h = 0; h < E::N; ++h) {
    any = any || on[h];
    all = all && (on[h] || (h == E::N - 1 && follow));
  }
  const bool keep = any && !all;   // a half is stored back as loaded
  R acc[E::N];
#pragma unroll
  for (int h = 0; h < E::N; ++h) acc[h] = 0;
  // (a slice whose elements all lie outside the block: nothing to load)
  if (__ballot(any) != 0)
    march_combine<R2, NS, nb_of(NS, E::N), serial_of(NS)>(p, off, cstep, nx, c, b.coef != nullptr, b.c0 != nullptr, b.clip != 0, on, follow, keep, acc);
  if (b.sum) {
#pragma unroll
    for (int h = 0; h < E::N; ++h)
      if (on[h]) static_cast<R*>(b.sum)[o[h]] = acc[h];
  }
}

// Reference layout: element (sl, column i, level k, tracer t) at f + sl + ld * ((i + 2) + (nx + 6) * (k + nlev * t));
// coef at bi + n * (k + nlev * j), c0 and sum at bi + n * k.  x: instances of the block, y: levels.
template <typename R, int NS>
__global__ void __launch_bounds__(256) ref_combine_kernel(R* f, const long long ld, const long long sl0, const long long n, const int nx,
                                                         const int nlev, const int dst, const Offs off, const R* coef, const R* c0,
                                                         const int clip, R* sum) {
  const long long bi = (long long)blockIdx.x * 256 + threadIdx.x;
  if (bi >= n) return;
  for (long long k = blockIdx.y; k < nlev; k += gridDim.y) {
    R* const p = f + (sl0 + bi) + ld * ((long long)(nx + 6) * (k + (long long)nlev * dst) + 3);   // column 1 of tracer dst
    const long long o = bi + n * k;
    Coef<R, NS> c;
#pragma unroll
    for (int j = 0; j < (NS > 0 ? NS : 1); ++j) c.cf[j] = (coef && NS > 0) ? coef[o + n * nlev * j] : (R)1;
    c.c0 = c0 ? c0[o] : (R)0;
    R acc = 0;
    for (int i = 0; i < nx; ++i) {
      R x[NS > 0 ? NS : 1];
#pragma unroll
      for (int j = 0; j < NS; ++j) x[j] = p[i * ld + off.o[j]];
      R v = 0;
#pragma unroll
      for (int j = 0; j < NS; ++j) combine_term<R, NS>(v, x[j], c, j, coef != nullptr);
      v = combine_tail<R, NS>(v, c, c0 != nullptr, clip != 0);
      p[i * ld] = v;
      acc = acc + v;
    }
    if (sum) sum[o] = acc;
  }
}

// launch(std::integral_constant<int, NS>{}) for NS = nsrc, so that a launch is written once
template <int NS = 0, typename F>
inline hipError_t with_nsrc(const int nsrc, F&& launch) {
  if (nsrc == NS) return launch(std::integral_constant<int, NS>{});
  if constexpr (NS < NSMAX) return with_nsrc<NS + 1>(nsrc, launch);
  return hipErrorInvalidValue;
}

}  // namespace

hipError_t mpdata_combine_wm(const MpdataCombineJob& job, hipStream_t stream) {
  WmGrid g;
  MpdataCombineJob b = job;
  if (b.dst < 0 || b.dst >= b.j.ntr || b.nsrc < 0 || b.nsrc > NSMAX || (b.nsrc == 0 && !b.c0)) return hipErrorInvalidValue;
  for (int q = 0; q < NSMAX; ++q) {
    if (q < b.nsrc && (b.src[q] < 0 || b.src[q] >= b.j.ntr)) return hipErrorInvalidValue;
    b.off[q] = q < b.nsrc ? (long long)(b.src[q] - b.dst) * b.j.prv_tstride : 0;
  }
  const hipError_t e = wm_block_grid(b.j, b.sel, 1, &g);
  if (e != hipSuccess) return e;
  return with_nsrc(b.nsrc, [&](auto ns) {
    constexpr int NS = decltype(ns)::value;
    return wm_block_launch(wm_combine_kernel<double, NS>, wm_combine_kernel<float2, NS>, b, g, stream);
  });
}

hipError_t mpdata_combine_ref(void* f, int elem_bytes, long long ld, long long sl0, long long n, int nx, int nlev, int ntr, int dst,
                              int nsrc, const int* src, const void* coef, const void* c0, int clip, void* sum, hipStream_t stream) {
  if (!f || ld < 1 || sl0 < 0 || n < 1 || sl0 + n > ld || nx < 1 || nlev < 1 || ntr < 1) return hipErrorInvalidValue;
  if (dst < 0 || dst >= ntr || nsrc < 0 || nsrc > NSMAX || (nsrc > 0 && !src) || (nsrc == 0 && !c0)) return hipErrorInvalidValue;
  Offs off;
  for (int q = 0; q < NSMAX; ++q) {
    if (q < nsrc && (src[q] < 0 || src[q] >= ntr)) return hipErrorInvalidValue;
    off.o[q] = q < nsrc ? ld * ((long long)(nx + 6) * nlev * (src[q] - dst)) : 0;   // signed
  }
  dim3 grid, block(256);
  if (ref_block_grid(n, nlev, &grid) != hipSuccess) return hipErrorInvalidValue;
  return ref_real(elem_bytes, [&](auto x) {
    typedef decltype(x) R;
    return with_nsrc(nsrc, [&](auto ns) {
      constexpr int NS = decltype(ns)::value;
      hipLaunchKernelGGL((ref_combine_kernel<R, NS>), grid, block, 0, stream, static_cast<R*>(f), ld, sl0, n, nx, nlev, dst, off,
                         static_cast<const R*>(coef), static_cast<const R*>(c0), clip, static_cast<R*>(sum));
      return hipGetLastError();
    });
  });
}
