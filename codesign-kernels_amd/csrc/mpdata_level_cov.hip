// mpdata_level_cov.hip -- per-level covariance of two tracers of f (include/mpdata_hip.h 3u, mpdata_level_cov.h): the sum
// over the interior columns 1 .. nx of (a_i - m_a) * (b_i - m_b), with m the given profile or the horizontal mean of the
// row itself, or of a_i * b_i (raw) -- horizontal variances and covariances, the amplitude that variance transport hands
// to a host model, second-moment statistics.  The first reduction that sees two tracers of a cell.  A kernel of its own
// outside the run: nothing is fused into the plan kernels, nothing is kept between calls, nothing of the plan is written.
//   plan layout: the walk of mpdata_wm_walk.h over the column slots 3 .. nx+2, a lane per element, as TWO read-only
//     streams -- tracer ta and, at a signed 64-bit offset from it, tracer tb (one stream where ta == tb) --, NB columns in
//     flight on each; the means and c are lane-local in column order.  Three forms with the same bits (mpdata_level_cov.h):
//     ONE-PASS (nothing to sum), KEPT (the columns stay in registers between the sum and the products), RE-READ (the
//     summing walk of mpdata_stats.hip, then the accumulating walk).  A lane reads the columns of its own element only, so
//     there is no LDS, no barrier and no ordering to argue.
//   reference layout: one thread per instance and level row, coalesced along sl, loops over i.
// Built with -ffp-contract=off and IEEE divides: every operation of the definition is rounded once, in its association.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "mpdata_level_cov.h"

namespace {

using namespace wm_walk;

// the limits of the KEPT form in columns: one stream (ta == tb) as mpdata_relax.hip's; two streams hold twice the data
// (-DMPDATA_LEVEL_COV_KEPT_NX1=0 -DMPDATA_LEVEL_COV_KEPT_NX2=0: the RE-READ form at every nx, for timing one form against
// the other: tools/level_cov_bench.py)
#ifndef MPDATA_LEVEL_COV_KEPT_NX1
#define MPDATA_LEVEL_COV_KEPT_NX1 32
#endif
#ifndef MPDATA_LEVEL_COV_KEPT_NX2
#define MPDATA_LEVEL_COV_KEPT_NX2 32
#endif
constexpr int KEPT_NX1 = MPDATA_LEVEL_COV_KEPT_NX1, KEPT_NX2 = MPDATA_LEVEL_COV_KEPT_NX2;
static_assert(KEPT_NX1 % NB == 0 && KEPT_NX2 % NB == 0 && KEPT_NX1 >= 0 && KEPT_NX2 >= 0, "the kept forms load whole groups of NB columns");
enum { ONE_PASS = 0, RE_READ = 1, KEPT = 2 };

// one column of the definition: p = da * db; c = c + p
template <typename R>
__device__ inline R cov_step(const R c, const R a, const R b, const R m_a, const R m_b, const bool raw) {
  const R da = raw ? a : a - m_a;
  const R db = raw ? b : b - m_b;
  const R p = da * db;
  return c + p;
}

// the sums of nx values p[0], p[step], ... (tracer ta; wanted: sa) and p[doff], p[doff + step], ... (tracer tb; wanted:
// sb) of every lane, s = +0; s = s + f_i: all loads of a batch are issued before the first is used (the index is
// clamped, not predicated); the batch's tail is cut by wave-uniform conditions.  !TWO: one stream, one sum for both.
template <typename R2, bool TWO>
__device__ inline void march_sum(const R2* p, const long long doff, const long long step, const int nx, const bool sa, const bool sb,
                                 typename Elem<R2>::R (&s_a)[Elem<R2>::N], typename Elem<R2>::R (&s_b)[Elem<R2>::N]) {
  typedef Elem<R2> E;
#pragma unroll
  for (int h = 0; h < E::N; ++h) { s_a[h] = 0; s_b[h] = 0; }
  const bool la = sa || !TWO, lb = TWO && sb;
  const R2* const pb = p + doff;
  for (int i = 0; i < nx; i += NB) {
    R2 va[NB], vb[NB];
    if (la) {
#pragma unroll
      for (int u = 0; u < NB; ++u) va[u] = p[(long long)min(i + u, nx - 1) * step];
    }
    if (lb) {
#pragma unroll
      for (int u = 0; u < NB; ++u) vb[u] = pb[(long long)min(i + u, nx - 1) * step];
    }
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      if (i + u < nx) {
#pragma unroll
        for (int h = 0; h < E::N; ++h) {
          if (la) s_a[h] = s_a[h] + E::get(va[u], h);
          if (lb) s_b[h] = s_b[h] + E::get(vb[u], h);
        }
      }
    }
  }
  if (!TWO) {
#pragma unroll
    for (int h = 0; h < E::N; ++h) s_b[h] = s_a[h];
  }
}

// c = +0; c = c + da_i * db_i over the same columns, i ascending: 2 NB loads in flight (NB where ta == tb)
template <typename R2, bool TWO>
__device__ inline void march_cov(const R2* p, const long long doff, const long long step, const int nx,
                                 const typename Elem<R2>::R (&m_a)[Elem<R2>::N], const typename Elem<R2>::R (&m_b)[Elem<R2>::N],
                                 const bool raw, typename Elem<R2>::R (&c)[Elem<R2>::N]) {
  typedef Elem<R2> E;
  typedef typename E::R R;
#pragma unroll
  for (int h = 0; h < E::N; ++h) c[h] = 0;
  const R2* const pb = p + doff;
  for (int i = 0; i < nx; i += NB) {
    R2 va[NB], vb[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) va[u] = p[(long long)min(i + u, nx - 1) * step];
    if (TWO) {
#pragma unroll
      for (int u = 0; u < NB; ++u) vb[u] = pb[(long long)min(i + u, nx - 1) * step];
    }
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      if (i + u < nx) {
#pragma unroll
        for (int h = 0; h < E::N; ++h) {
          const R a = E::get(va[u], h);
          const R b = TWO ? E::get(vb[u], h) : a;
          c[h] = cov_step<R>(c[h], a, b, m_a[h], m_b[h], raw);
        }
      }
    }
  }
}

// The KEPT form, nx <= KNX: the columns of the lane's element stay in registers between the sums and the products, so f
// is loaded once.  Fully unrolled and statically indexed (no scratch); the loads go out in groups of NB with the index
// clamped inside a group, the groups cut by wave-uniform conditions.  Sums, divides and products are those of march_sum
// and march_cov, in the same order: the same bits.  m_a, m_b: the given profiles on entry where !sa, !sb; the means used
// on return.
template <typename R2, bool TWO, int KNX>
__device__ inline void march_kept(const R2* p, const long long doff, const long long step, const int nx, const bool sa, const bool sb,
                                  typename Elem<R2>::R (&m_a)[Elem<R2>::N], typename Elem<R2>::R (&m_b)[Elem<R2>::N],
                                  typename Elem<R2>::R (&c)[Elem<R2>::N]) {
  typedef Elem<R2> E;
  typedef typename E::R R;
  constexpr int KB = TWO ? KNX : 1;
  R2 va[KNX], vb[KB];
  const R2* const pb = p + doff;
#pragma unroll
  for (int g = 0; g < KNX; g += NB) {
    if (g < nx) {
#pragma unroll
      for (int u = 0; u < NB; ++u) va[g + u] = p[(long long)min(g + u, nx - 1) * step];
      if (TWO) {
#pragma unroll
        for (int u = 0; u < NB; ++u) vb[TWO ? g + u : 0] = pb[(long long)min(g + u, nx - 1) * step];
      }
    }
  }
  R s_a[E::N], s_b[E::N];
#pragma unroll
  for (int h = 0; h < E::N; ++h) { s_a[h] = 0; s_b[h] = 0; }
#pragma unroll
  for (int i = 0; i < KNX; ++i) {
    if (i < nx) {
#pragma unroll
      for (int h = 0; h < E::N; ++h) {
        s_a[h] = s_a[h] + E::get(va[i], h);
        if (TWO) s_b[h] = s_b[h] + E::get(vb[TWO ? i : 0], h);
      }
    }
  }
  const R rnx = (R)nx;   // exact: nx < 2^24
#pragma unroll
  for (int h = 0; h < E::N; ++h) {
    if (!TWO) s_b[h] = s_a[h];
    if (sa) m_a[h] = s_a[h] / rnx;
    if (sb) m_b[h] = s_b[h] / rnx;
    c[h] = 0;
  }
#pragma unroll
  for (int i = 0; i < KNX; ++i) {
    if (i < nx) {
#pragma unroll
      for (int h = 0; h < E::N; ++h) {
        const R a = E::get(va[i], h);
        const R b = TWO ? E::get(vb[TWO ? i : 0], h) : a;
        c[h] = cov_step<R>(c[h], a, b, m_a[h], m_b[h], false);
      }
    }
  }
}

// Plan layout: a wave per (tile of the block, 64-element slice of the chunk), lane -> element e = s * nlev + kk.
// R2: one 8-byte element (double, or the float2 of two adjacent slots); FORM: ONE_PASS, RE_READ or KEPT; TWO: ta != tb.
template <typename R2, int FORM, bool TWO>
__global__ void __launch_bounds__(256) wm_level_cov_kernel(const MpdataLevelCovJob b, const long long t0, const int ntile, const int nslice) {
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
  const R2* p = static_cast<const R2*>(j.prv) + (long long)b.ta * j.prv_tstride + tile * j.prv_tile_stride +
                (in_main ? e : (long long)j.ncol_p * j.main_e + (e - j.main_e)) + 3 * cstep;   // column 1 = slot 3
  const long long doff = TWO ? (long long)(b.tb - b.ta) * j.prv_tstride : 0;                   // signed: tb < ta walks back
  // per half: the instance and the tall level the slot stands for, its given means and its place in the arrays
  const int nzm = b.sel.nz - 1;
  R m_a[E::N], m_b[E::N];
  bool in[E::N];
  long long o[E::N];
  bool any = false;
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
      ok = ok && k + 1 >= own0 && k + 1 <= own1;   // the level's owner alone reads it
    }
    // else: padding, the phantom, the partner of a split pair, a neighbour in the tile
    ok = ok && sl >= b.sel.sl0 && sl < b.sel.sl0 + b.sel.n && k < nzm;
    in[h] = ok;
    any = any || ok;
    o[h] = ok ? (sl - b.sel.sl0) + b.sel.n * (long long)k : 0;
    m_a[h] = (b.ma && ok) ? static_cast<const R*>(b.ma)[o[h]] : (R)0;
    m_b[h] = (b.mb && ok) ? static_cast<const R*>(b.mb)[o[h]] : (R)0;
  }
  if (__ballot(any) == 0) return;   // (a slice none of whose elements is in the block, or owned: nothing to load)
  R c[E::N];
  if (FORM == ONE_PASS) {
    march_cov<R2, TWO>(p, doff, cstep, nx, m_a, m_b, b.raw != 0, c);
  } else {
    const bool sa = b.ma == nullptr, sb = b.mb == nullptr;
    if (FORM == KEPT) {
      constexpr int KNX = TWO ? KEPT_NX2 : KEPT_NX1;   // (0: the form is not launched; NB only keeps the arrays legal)
      march_kept<R2, TWO, (KNX > 0 ? KNX : NB)>(p, doff, cstep, nx, sa, sb, m_a, m_b, c);
    } else {
      R s_a[E::N], s_b[E::N];
      march_sum<R2, TWO>(p, doff, cstep, nx, sa, sb, s_a, s_b);
      const R rnx = (R)nx;   // exact: nx < 2^24
#pragma unroll
      for (int h = 0; h < E::N; ++h) {
        if (sa) m_a[h] = s_a[h] / rnx;
        if (sb) m_b[h] = s_b[h] / rnx;
      }
      march_cov<R2, TWO>(p, doff, cstep, nx, m_a, m_b, false, c);
    }
  }
#pragma unroll
  for (int h = 0; h < E::N; ++h) {
    if (!in[h]) continue;
    static_cast<R*>(b.cov)[o[h]] = c[h];
    if (b.mean_a) static_cast<R*>(b.mean_a)[o[h]] = m_a[h];
    if (b.mean_b) static_cast<R*>(b.mean_b)[o[h]] = m_b[h];
  }
}

// Reference layout: element (sl, column i, level k, tracer t) at f + sl + ld * ((i + 2) + (nx + 6) * (k + nlev * t)); ma,
// mb, cov, mean_a, mean_b at bi + n * k.  x: instances of the block, y: levels.
template <typename R>
__global__ void __launch_bounds__(256) ref_level_cov_kernel(const R* f, const long long ld, const long long sl0, const long long n,
                                                           const int nx, const int nlev, const int ta, const int tb, const R* ma,
                                                           const R* mb, const int raw, R* cov, R* mean_a, R* mean_b) {
  const long long bi = (long long)blockIdx.x * 256 + threadIdx.x;
  if (bi >= n) return;
  const long long doff = ld * ((long long)(nx + 6) * nlev * (tb - ta));   // signed
  const bool sa = !raw && !ma, sb = !raw && !mb;
  for (long long k = blockIdx.y; k < nlev; k += gridDim.y) {
    const R* const p = f + (sl0 + bi) + ld * ((long long)(nx + 6) * (k + (long long)nlev * ta) + 3);   // column 1 of tracer ta
    const long long o = bi + n * k;
    R m_a[1] = {ma ? ma[o] : (R)0}, m_b[1] = {mb ? mb[o] : (R)0}, c[1];
    if (sa || sb) {
      R s_a[1], s_b[1];
      march_sum<R, true>(p, doff, ld, nx, sa, sb, s_a, s_b);
      if (sa) m_a[0] = s_a[0] / (R)nx;
      if (sb) m_b[0] = s_b[0] / (R)nx;
    }
    march_cov<R, true>(p, doff, ld, nx, m_a, m_b, raw != 0, c);
    cov[o] = c[0];
    if (mean_a) mean_a[o] = m_a[0];
    if (mean_b) mean_b[o] = m_b[0];
  }
}

template <int FORM, bool TWO>
hipError_t launch_form(const MpdataLevelCovJob& b, const WmGrid& g, hipStream_t stream) {
  return wm_block_launch(wm_level_cov_kernel<double, FORM, TWO>, wm_level_cov_kernel<float2, FORM, TWO>, b, g, stream);
}

bool bad_args(int ntr, int ta, int tb, const void* ma, const void* mb, int raw, const void* cov, const void* mean_a, const void* mean_b) {
  return !cov || ta < 0 || tb < 0 || ta >= ntr || tb >= ntr || (raw && (ma || mb || mean_a || mean_b));
}

}  // namespace

hipError_t mpdata_level_cov_wm(const MpdataLevelCovJob& b, hipStream_t stream) {
  WmGrid g;
  if (bad_args(b.j.ntr, b.ta, b.tb, b.ma, b.mb, b.raw, b.cov, b.mean_a, b.mean_b)) return hipErrorInvalidValue;
  const hipError_t e = wm_block_grid(b.j, b.sel, 1, &g);
  if (e != hipSuccess) return e;
  const bool two = b.ta != b.tb;
  const int nx = b.j.ncol_p - 6;
  if (b.raw || (b.ma && b.mb))   // nothing to sum
    return two ? launch_form<ONE_PASS, true>(b, g, stream) : launch_form<ONE_PASS, false>(b, g, stream);
  if (nx <= (two ? KEPT_NX2 : KEPT_NX1))   // the columns fit the registers: f is loaded once
    return two ? launch_form<KEPT, true>(b, g, stream) : launch_form<KEPT, false>(b, g, stream);
  return two ? launch_form<RE_READ, true>(b, g, stream) : launch_form<RE_READ, false>(b, g, stream);
}

hipError_t mpdata_level_cov_ref(const void* f, int elem_bytes, long long ld, long long sl0, long long n, int nx, int nlev, int ntr,
                                int ta, int tb, const void* ma, const void* mb, int raw, void* cov, void* mean_a, void* mean_b,
                                hipStream_t stream) {
  if (!f || ld < 1 || sl0 < 0 || n < 1 || sl0 + n > ld || nx < 1 || nlev < 1 || ntr < 1) return hipErrorInvalidValue;
  if (bad_args(ntr, ta, tb, ma, mb, raw, cov, mean_a, mean_b)) return hipErrorInvalidValue;
  dim3 grid, block(256);
  if (ref_block_grid(n, nlev, &grid) != hipSuccess) return hipErrorInvalidValue;
  return ref_real(elem_bytes, [&](auto x) {
    typedef decltype(x) R;
    hipLaunchKernelGGL((ref_level_cov_kernel<R>), grid, block, 0, stream, static_cast<const R*>(f), ld, sl0, n, nx, nlev, ta, tb,
                       static_cast<const R*>(ma), static_cast<const R*>(mb), raw, static_cast<R*>(cov), static_cast<R*>(mean_a),
                       static_cast<R*>(mean_b));
    return hipGetLastError();
  });
}
