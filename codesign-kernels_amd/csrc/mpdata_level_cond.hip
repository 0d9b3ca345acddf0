// mpdata_level_cond.hip -- per-level conditional counts and sums of the tracers of f (include/mpdata_hip.h 3v,
// mpdata_level_cond.h): how many interior columns 1 .. nx of a level have the condition tracer inside (lo, hi], and the sum
// of every value tracer over exactly those columns -- cloud fraction and in-cloud means, core and environment averages, a
// histogram bin by bin.  A kernel of its own outside the run: nothing is fused into the plan kernels, nothing is kept
// between calls, nothing of the plan is written.
//   plan layout: the walk of mpdata_wm_walk.h over the column slots 3 .. nx+2, a lane per element, NB columns in flight;
//     the value tracers lie at signed 64-bit offsets from the tc stream and are a loop inside the kernel.  Two forms with
//     the same bits (mpdata_level_cond.h): MASK (the condition is read once and kept as a 64-bit mask per lane) and
//     RE-READ (the condition is read and compared again with every value tracer).  A lane reads the columns of its own
//     element only, so there is no LDS, no barrier and no ordering to argue.
//   reference layout: one thread per instance and level row, coalesced along sl, loops over i.
// A column that is not in is selected away (s = in ? s + v : s), never multiplied away: an excluded infinity or NaN of a
// value tracer does not reach a sum.  Built with -ffp-contract=off: every add is rounded once, in column order.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "mpdata_level_cond.h"

namespace {

using namespace wm_walk;

// the limit of the MASK form in columns: the mask of a lane and half is two 32-bit registers
// (-DMPDATA_LEVEL_COND_MASK_NX=0: the RE-READ form at every nx, for timing one form against the other:
// tools/level_cond_bench.py)
#ifndef MPDATA_LEVEL_COND_MASK_NX
#define MPDATA_LEVEL_COND_MASK_NX 64
#endif
constexpr int MASK_NX = MPDATA_LEVEL_COND_MASK_NX;
static_assert(MASK_NX >= 0 && MASK_NX <= 64, "a mask bit per column");
enum { RE_READ = 0, MASK = 1 };

// in_i: plain compares; an absent bound holds for every column
template <typename R>
__device__ inline bool is_in(const R c, const R lo, const R hi, const bool has_lo, const bool has_hi) {
  return (!has_lo || c > lo) && (!has_hi || c <= hi);
}

// The RE-READ walk: q = +0, s = +0; over the columns p[0], p[step], ... of the condition (and p[doff], p[doff + step], ...
// of the value tracer; !TWO: the condition is the value), i ascending: if in_i: q = q + 1; s = s + v_i.  All loads of a
// batch are issued before the first is used (the index is clamped, not predicated); the batch's tail is cut by
// wave-uniform conditions.
template <typename R2, bool TWO>
__device__ inline void march_cond(const R2* p, const long long doff, const long long step, const int nx,
                                  const typename Elem<R2>::R (&lo)[Elem<R2>::N], const typename Elem<R2>::R (&hi)[Elem<R2>::N],
                                  const bool has_lo, const bool has_hi, typename Elem<R2>::R (&q)[Elem<R2>::N],
                                  typename Elem<R2>::R (&s)[Elem<R2>::N]) {
  typedef Elem<R2> E;
  typedef typename E::R R;
#pragma unroll
  for (int h = 0; h < E::N; ++h) { q[h] = 0; s[h] = 0; }
  const R2* const pv = p + doff;
  for (int i = 0; i < nx; i += NB) {
    R2 vc[NB], vv[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) vc[u] = p[(long long)min(i + u, nx - 1) * step];
    if (TWO) {
#pragma unroll
      for (int u = 0; u < NB; ++u) vv[u] = pv[(long long)min(i + u, nx - 1) * step];
    }
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      if (i + u < nx) {
#pragma unroll
        for (int h = 0; h < E::N; ++h) {
          const R c = E::get(vc[u], h);
          const R v = TWO ? E::get(vv[u], h) : c;
          const bool in = is_in<R>(c, lo[h], hi[h], has_lo, has_hi);
          q[h] = in ? q[h] + (R)1 : q[h];
          s[h] = in ? s[h] + v : s[h];
        }
      }
    }
  }
}

// The MASK form, nx <= 64.  First walk, over the condition: q and s as march_cond<R2, false> forms them, and bit i of
// (m0, m1) = in_i (bits of columns >= nx stay 0).  A batch of NB columns makes one byte of the mask with compile-time bit
// positions, shifted to its place in the word by a wave-uniform amount: the two words are plain registers, never an array
// that is indexed at run time.
template <typename R2>
__device__ inline void mask_walk(const R2* p, const long long step, const int nx, const typename Elem<R2>::R (&lo)[Elem<R2>::N],
                                 const typename Elem<R2>::R (&hi)[Elem<R2>::N], const bool has_lo, const bool has_hi,
                                 unsigned (&m0)[Elem<R2>::N], unsigned (&m1)[Elem<R2>::N], typename Elem<R2>::R (&q)[Elem<R2>::N],
                                 typename Elem<R2>::R (&s)[Elem<R2>::N]) {
  typedef Elem<R2> E;
  typedef typename E::R R;
  static_assert(NB == 8, "a batch is a byte of the mask");
#pragma unroll
  for (int h = 0; h < E::N; ++h) { q[h] = 0; s[h] = 0; m0[h] = 0; m1[h] = 0; }
#pragma nounroll
  for (int g = 0; g < nx; g += NB) {
    R2 vc[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) vc[u] = p[(long long)min(g + u, nx - 1) * step];
    unsigned byte[E::N];
#pragma unroll
    for (int h = 0; h < E::N; ++h) byte[h] = 0;
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      if (g + u < nx) {
#pragma unroll
        for (int h = 0; h < E::N; ++h) {
          const R c = E::get(vc[u], h);
          const bool in = is_in<R>(c, lo[h], hi[h], has_lo, has_hi);
          q[h] = in ? q[h] + (R)1 : q[h];
          s[h] = in ? s[h] + c : s[h];
          byte[h] |= in ? 1u << u : 0u;
        }
      }
    }
    const int sh = g & 31;
#pragma unroll
    for (int h = 0; h < E::N; ++h) {
      if (g < 32) m0[h] |= byte[h] << sh; else m1[h] |= byte[h] << sh;
    }
  }
}
// ... and the walk of a value tracer under the mask: s = +0; if bit i: s = s + v_i, i ascending (a clamped load beyond nx
// meets a 0 bit)
template <typename R2>
__device__ inline void mask_sum(const R2* p, const long long step, const int nx, const unsigned (&m0)[Elem<R2>::N],
                                const unsigned (&m1)[Elem<R2>::N], typename Elem<R2>::R (&s)[Elem<R2>::N]) {
  typedef Elem<R2> E;
#pragma unroll
  for (int h = 0; h < E::N; ++h) s[h] = 0;
#pragma nounroll
  for (int g = 0; g < nx; g += NB) {
    R2 vv[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) vv[u] = p[(long long)min(g + u, nx - 1) * step];
    unsigned byte[E::N];
#pragma unroll
    for (int h = 0; h < E::N; ++h) byte[h] = (g < 32 ? m0[h] : m1[h]) >> (g & 31);
#pragma unroll
    for (int u = 0; u < NB; ++u) {
#pragma unroll
      for (int h = 0; h < E::N; ++h) {
        const bool in = (byte[h] >> u) & 1u;
        s[h] = in ? s[h] + E::get(vv[u], h) : s[h];
      }
    }
  }
}

// Plan layout: a wave per (tile of the block, 64-element slice of the chunk), lane -> element e = s * nlev + kk.
// (The head of the kernel down to the ballot has a twin, hist_rows of mpdata_level_hist.hip: a change to either belongs in both.)
// R2: one 8-byte element (double, or the float2 of two adjacent slots); FORM: MASK or RE_READ.
template <typename R2, int FORM>
__global__ void __launch_bounds__(256) wm_level_cond_kernel(const MpdataLevelCondJob b, const long long t0, const int ntile, const int nslice) {
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
  const R2* p = static_cast<const R2*>(j.prv) + (long long)b.tc * j.prv_tstride + tile * j.prv_tile_stride +
                (in_main ? e : (long long)j.ncol_p * j.main_e + (e - j.main_e)) + 3 * cstep;   // column 1 = slot 3
  // per half: the instance and the tall level the slot stands for, its bounds and its place in the arrays
  const int nzm = b.sel.nz - 1;
  const bool has_lo = b.lo != nullptr, has_hi = b.hi != nullptr;
  R lo[E::N], hi[E::N];
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
    lo[h] = (has_lo && ok) ? static_cast<const R*>(b.lo)[o[h]] : (R)0;
    hi[h] = (has_hi && ok) ? static_cast<const R*>(b.hi)[o[h]] : (R)0;
  }
  if (__ballot(any) == 0) return;   // (a slice none of whose elements is in the block, or owned: nothing to load)
  const long long nout = b.sel.n * (long long)nzm;   // csum(b, k, j): one (n, nzm) array per value tracer
  const int ntr = b.csum ? b.ntr : 0;
  R q[E::N], sc[E::N];
  if (FORM == MASK) {
    unsigned m0[E::N], m1[E::N];
    mask_walk<R2>(p, cstep, nx, lo, hi, has_lo, has_hi, m0, m1, q, sc);
    if (b.cnt) {
#pragma unroll
      for (int h = 0; h < E::N; ++h)
        if (in[h]) static_cast<R*>(b.cnt)[o[h]] = q[h];
    }
    for (int jt = 0; jt < ntr; ++jt) {
      const int t = b.first + jt;
      R sv[E::N];
      if (t == b.tc) {   // the first walk summed it
#pragma unroll
        for (int h = 0; h < E::N; ++h) sv[h] = sc[h];
      } else {
        mask_sum<R2>(p + (long long)(t - b.tc) * j.prv_tstride, cstep, nx, m0, m1, sv);   // signed: t < tc walks back
      }
#pragma unroll
      for (int h = 0; h < E::N; ++h)
        if (in[h]) static_cast<R*>(b.csum)[o[h] + nout * jt] = sv[h];
    }
  } else {
    if (ntr == 0) march_cond<R2, false>(p, 0, cstep, nx, lo, hi, has_lo, has_hi, q, sc);
    for (int jt = 0; jt < ntr; ++jt) {
      const int t = b.first + jt;
      if (t == b.tc)
        march_cond<R2, false>(p, 0, cstep, nx, lo, hi, has_lo, has_hi, q, sc);
      else
        march_cond<R2, true>(p, (long long)(t - b.tc) * j.prv_tstride, cstep, nx, lo, hi, has_lo, has_hi, q, sc);
#pragma unroll
      for (int h = 0; h < E::N; ++h)
        if (in[h]) static_cast<R*>(b.csum)[o[h] + nout * jt] = sc[h];
    }
    if (b.cnt) {   // (every walk forms the same q)
#pragma unroll
      for (int h = 0; h < E::N; ++h)
        if (in[h]) static_cast<R*>(b.cnt)[o[h]] = q[h];
    }
  }
}

// Reference layout: element (sl, column i, level k, tracer t) at f + sl + ld * ((i + 2) + (nx + 6) * (k + nlev * t)); lo,
// hi, cnt at bi + n * k, csum at bi + n * (k + nlev * j).  x: instances of the block, y: levels.
template <typename R>
__global__ void __launch_bounds__(256) ref_level_cond_kernel(const R* f, const long long ld, const long long sl0, const long long n,
                                                            const int nx, const int nlev, const int tc, const R* lo, const R* hi, R* cnt,
                                                            R* csum, const int first, const int ntr) {
  const long long bi = (long long)blockIdx.x * 256 + threadIdx.x;
  if (bi >= n) return;
  const long long tstride = ld * ((long long)(nx + 6) * nlev);
  const bool has_lo = lo != nullptr, has_hi = hi != nullptr;
  for (long long k = blockIdx.y; k < nlev; k += gridDim.y) {
    const R* const p = f + (sl0 + bi) + ld * ((long long)(nx + 6) * (k + (long long)nlev * tc) + 3);   // column 1 of tracer tc
    const long long o = bi + n * k;
    const R l[1] = {has_lo ? lo[o] : (R)0}, h[1] = {has_hi ? hi[o] : (R)0};
    R q[1], s[1];
    if (ntr == 0) march_cond<R, false>(p, 0, ld, nx, l, h, has_lo, has_hi, q, s);
    for (int jt = 0; jt < ntr; ++jt) {
      const int t = first + jt;
      if (t == tc)
        march_cond<R, false>(p, 0, ld, nx, l, h, has_lo, has_hi, q, s);
      else
        march_cond<R, true>(p, tstride * (t - tc), ld, nx, l, h, has_lo, has_hi, q, s);   // signed
      csum[o + n * nlev * jt] = s[0];
    }
    if (cnt) cnt[o] = q[0];
  }
}

bool bad_args(int ntr_all, int tc, const void* lo, const void* hi, const void* cnt, const void* csum, int first, int ntr) {
  return tc < 0 || tc >= ntr_all || (!lo && !hi) || (!cnt && !csum) || (csum && (first < 0 || ntr < 1 || first > ntr_all - ntr));
}

}  // namespace

hipError_t mpdata_level_cond_wm(const MpdataLevelCondJob& b, hipStream_t stream) {
  WmGrid g;
  if (bad_args(b.j.ntr, b.tc, b.lo, b.hi, b.cnt, b.csum, b.first, b.ntr)) return hipErrorInvalidValue;
  const hipError_t e = wm_block_grid(b.j, b.sel, 1, &g);
  if (e != hipSuccess) return e;
  // a mask bit per column and the condition read once pay from two value tracers on; cnt alone and one value tracer read
  // the same bytes in either form, and there RE-READ is the faster one or as fast (docs/EXPERIMENTS.md AF)
  if (b.j.ncol_p - 6 <= MASK_NX && b.csum && b.ntr >= 2)
    return wm_block_launch(wm_level_cond_kernel<double, MASK>, wm_level_cond_kernel<float2, MASK>, b, g, stream);
  return wm_block_launch(wm_level_cond_kernel<double, RE_READ>, wm_level_cond_kernel<float2, RE_READ>, b, g, stream);
}

hipError_t mpdata_level_cond_ref(const void* f, int elem_bytes, long long ld, long long sl0, long long n, int nx, int nlev, int ntr_all,
                                 int tc, const void* lo, const void* hi, void* cnt, void* csum, int first, int ntr, hipStream_t stream) {
  if (!f || ld < 1 || sl0 < 0 || n < 1 || sl0 + n > ld || nx < 1 || nlev < 1 || ntr_all < 1) return hipErrorInvalidValue;
  if (bad_args(ntr_all, tc, lo, hi, cnt, csum, first, ntr)) return hipErrorInvalidValue;
  dim3 grid, block(256);
  if (ref_block_grid(n, nlev, &grid) != hipSuccess) return hipErrorInvalidValue;
  return ref_real(elem_bytes, [&](auto x) {
    typedef decltype(x) R;
    hipLaunchKernelGGL((ref_level_cond_kernel<R>), grid, block, 0, stream, static_cast<const R*>(f), ld, sl0, n, nx, nlev, tc,
                       static_cast<const R*>(lo), static_cast<const R*>(hi), static_cast<R*>(cnt), static_cast<R*>(csum), first,
                       csum ? ntr : 0);
    return hipGetLastError();
  });
}
