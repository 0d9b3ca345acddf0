// mpdata_level_draft.hip -- per-level updraft / downdraft sampling of the tracers of f by the cell-centred vertical velocity
// (include/mpdata_hip.h 3ac, mpdata_level_draft.h): every interior column 1 .. nx of a level is put into one of three
// classes by wc = 0.5 * (w(k) + w(k+1)) against two thresholds -- UP, DOWN, ENV --, optionally only where a condition tracer
// lies inside (lo, hi], and per class the columns are counted and wc, every value tracer and wc * tracer are summed: SAM's
// core / downdraft / environment averages, the cloudy and unsaturated up and down mass fluxes an MMF hands back, the
// resolved flux split by draft.  A kernel of its own outside the run: nothing is fused into the plan kernels, nothing is
// kept between calls, nothing of the plan is written.
//   plan layout: the lane-owned walk of mpdata_level_cond.hip over the column slots 3 .. nx+2 of f, with the two w streams
//     of mpdata_courant.hip beside it (w(k+1) is element e + 1 of the same column, through an address and a stride of its
//     own); the value tracers lie at signed 64-bit offsets from the tc stream and are a loop inside the kernel, a GROUP of
//     4, 2 or 1 of them per walk.  ONE form: the class is formed again in every walk.  A lane reads the columns of its own
//     element only, so there is no LDS, no barrier and no ordering to argue.
//   reference layout: one thread per instance and level row, coalesced along sl, loops over i, one value tracer a walk.
// A column outside a class is selected away (s = is ? s + v : s), never multiplied away.  Built with -ffp-contract=off:
// every add and the product wc * v are rounded once, in column order.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "mpdata_level_draft.h"

namespace {

using namespace wm_walk;

constexpr int NC = MPDATA_LEVEL_DRAFT_CLASSES;
enum { UP = 0, DOWN = 1, ENV = 2 };

// columns in flight of a walk of G value tracers: 3 + G streams of 8-byte elements a column
template <int G> struct Batch { static constexpr int NBG = G >= 4 ? 4 : NB; };

// the accumulators of a lane: per half and class; GA value tracers.  Indexed by unrolled loops only.
template <typename R, int N, int GA>
struct Acc {
  unsigned q[N][NC];
  R ws[N][NC];
  R fs[N][NC][GA];
  R wf[N][NC][GA];
};

// what a walk needs beside its streams
template <typename R, int N>
struct Cond {
  R lo[N], hi[N];
  bool hasc, has_lo, has_hi, top;
  R wup, wdn;
};

// The walk over the columns pw0[0], pw0[su], ... of w(k), pw1[0], pw1[sw1], ... of w(k+1) (top: not used, +0 is taken),
// pc[0], pc[su], ... of the condition (hasc: else not loaded) and pv[g * tstr + i * su] of G value tracers, i ascending:
// CW: q[c] = q[c] + 1, ws[c] = ws[c] + wc; fs[c][g] = fs[c][g] + v; WF: p = wc * v, wf[c][g] = wf[c][g] + p, each for
// the one class c of the column.  All loads of a batch are issued before the first is used (the index is clamped, not
// predicated); the batch's tail is cut by wave-uniform conditions.
template <typename R2, int G, bool CW, bool WF>
__device__ inline void march_draft(const R2* pw0, const R2* pw1, const R2* pc, const R2* pv, const long long tstr, const long long su,
                                   const long long sw1, const int nx, const Cond<typename Elem<R2>::R, Elem<R2>::N>& cd,
                                   Acc<typename Elem<R2>::R, Elem<R2>::N, (G > 0 ? G : 1)>& a) {
  typedef Elem<R2> E;
  typedef typename E::R R;
  constexpr int NBG = Batch<G>::NBG, GA = G > 0 ? G : 1;
#pragma unroll
  for (int h = 0; h < E::N; ++h) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      a.q[h][c] = 0;
      a.ws[h][c] = 0;
#pragma unroll
      for (int g = 0; g < GA; ++g) { a.fs[h][c][g] = 0; a.wf[h][c][g] = 0; }
    }
  }
#pragma nounroll
  for (int i = 0; i < nx; i += NBG) {
    R2 wv[NBG], wn[NBG], vc[NBG], vv[GA][NBG];
#pragma unroll
    for (int u = 0; u < NBG; ++u) {
      const long long c = min(i + u, nx - 1);
      wv[u] = pw0[c * su];
      wn[u] = pw1[c * sw1];
    }
    if (cd.hasc) {
#pragma unroll
      for (int u = 0; u < NBG; ++u) vc[u] = pc[(long long)min(i + u, nx - 1) * su];
    } else {
#pragma unroll
      for (int u = 0; u < NBG; ++u) vc[u] = wv[u];   // (never compared)
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
      for (int u = 0; u < NBG; ++u) vv[g][u] = pv[g * tstr + (long long)min(i + u, nx - 1) * su];
    }
#pragma unroll
    for (int u = 0; u < NBG; ++u) {
      if (i + u < nx) {
#pragma unroll
        for (int h = 0; h < E::N; ++h) {
          const R wk1 = cd.top ? (R)0 : E::get(wn[u], h);
          const R s = E::get(wv[u], h) + wk1;
          const R wc = (R)0.5 * s;
          const R c = E::get(vc[u], h);
          const bool in = !cd.hasc || ((!cd.has_lo || c > cd.lo[h]) && (!cd.has_hi || c <= cd.hi[h]));
          const bool up = wc > cd.wup, dn = wc < cd.wdn;
          const bool is[NC] = {in && up, in && dn, in && !up && !dn};
#pragma unroll
          for (int k = 0; k < NC; ++k) {
            if (CW) {
              a.q[h][k] += is[k] ? 1u : 0u;
              a.ws[h][k] = is[k] ? a.ws[h][k] + wc : a.ws[h][k];
            }
#pragma unroll
            for (int g = 0; g < G; ++g) {
              const R v = E::get(vv[g][u], h);
              a.fs[h][k][g] = is[k] ? a.fs[h][k][g] + v : a.fs[h][k][g];
              if (WF) {
                const R p = wc * v;
                a.wf[h][k][g] = is[k] ? a.wf[h][k][g] + p : a.wf[h][k][g];
              }
            }
          }
        }
      }
    }
  }
}

// what a lane of the plan-layout kernel owns: per half whether it is an output row of the block and where the row lies
template <int N>
struct Rows {
  bool in[N];
  long long o[N];
};

// the streams of a lane of the plan-layout kernel
template <typename R2>
struct Streams {
  const R2 *pw0, *pw1, *pf;   // w(k), w(k+1), tracer max(tc, 0) of f: each at column 1
  long long su, sw1;
};

// one walk of the plan-layout kernel over the value tracers [t, t + G) and its stores; CW: it also stores cnt and wsum
template <typename R2, int G, bool CW, bool WF>
__device__ inline void walk_wm(const MpdataLevelDraftJob& b, const Streams<R2>& st, const int nx,
                               const Cond<typename Elem<R2>::R, Elem<R2>::N>& cd, const Rows<Elem<R2>::N>& r, const int jt) {
  typedef Elem<R2> E;
  typedef typename E::R R;
  constexpr int GA = G > 0 ? G : 1;
  const long long tstr = b.j.prv_tstride;
  const int tcb = b.tc < 0 ? 0 : b.tc;
  Acc<R, E::N, GA> a;
  march_draft<R2, G, CW, WF>(st.pw0, st.pw1, st.pf, st.pf + (long long)(b.first + jt - tcb) * tstr, tstr, st.su, st.sw1, nx, cd, a);
  const long long nout = b.sel.n * (long long)(b.sel.nz - 1);   // one (n, nzm) array per class and value tracer
#pragma unroll
  for (int h = 0; h < E::N; ++h) {
    if (!r.in[h]) continue;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      if (CW && b.cnt) static_cast<R*>(b.cnt)[r.o[h] + nout * k] = (R)a.q[h][k];   // exact: nx < 2^24
      if (CW && b.wsum) static_cast<R*>(b.wsum)[r.o[h] + nout * k] = a.ws[h][k];
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const long long o = r.o[h] + nout * (k + (long long)NC * (jt + g));
        if (b.fsum) static_cast<R*>(b.fsum)[o] = a.fs[h][k][g];
        if (WF) static_cast<R*>(b.wfsum)[o] = a.wf[h][k][g];
      }
    }
  }
}

// Plan layout: a wave per (tile of the block, 64-element slice of the chunk), lane -> element e = s * nlev + kk.
// (The head down to the ballot follows wm_level_cond_kernel, mpdata_level_cond.hip, and for the two w streams
// wm_courant_kernel, mpdata_courant.hip: the same lanes, windows, pairs and block test.)
// R2: one 8-byte element (double, or the float2 of two adjacent slots); WF: wfsum is wanted.
template <typename R2, bool WF>
__global__ void __launch_bounds__(256) wm_level_draft_kernel(const MpdataLevelDraftJob b, const long long t0, const int ntile, const int nslice) {
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
  const bool top = kk + 1 == nlev;
  const int e1 = top ? e : e + 1;
  const long long rem_e = j.chunk - j.main_e;
  const bool main0 = e < j.main_e, main1 = e1 < j.main_e;
  Streams<R2> st;
  st.su = main0 ? j.main_e : rem_e;
  st.sw1 = main1 ? j.main_e : rem_e;
  const long long tb = tile * j.prv_tile_stride;
  const long long o0 = tb + (main0 ? e : (long long)j.ncol_p * j.main_e + (e - j.main_e)) + 3 * st.su;      // column 1 = slot 3
  const long long o1 = tb + (main1 ? e1 : (long long)j.ncol_p * j.main_e + (e1 - j.main_e)) + 3 * st.sw1;
  const int tcb = b.tc < 0 ? 0 : b.tc;
  st.pw0 = static_cast<const R2*>(b.w) + o0;
  st.pw1 = static_cast<const R2*>(b.w) + o1;
  st.pf = static_cast<const R2*>(j.prv) + (long long)tcb * j.prv_tstride + o0;
  // per half: the instance and the tall level the slot stands for, its bounds and its place in the arrays
  const int nzm = b.sel.nz - 1;
  Cond<R, E::N> cd;
  cd.hasc = b.tc >= 0;
  cd.has_lo = b.lo != nullptr; cd.has_hi = b.hi != nullptr;
  cd.top = top;
  cd.wup = (R)b.wup; cd.wdn = (R)b.wdn;   // rounded once
  Rows<E::N> r;
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
      ok = ok && k + 1 >= own0 && k + 1 <= own1;   // the level's owner alone reads it (its k + 1 lies inside its window)
    }
    // else: padding, the phantom, the partner of a split pair, a neighbour in the tile
    ok = ok && sl >= b.sel.sl0 && sl < b.sel.sl0 + b.sel.n && k < nzm;
    r.in[h] = ok;
    any = any || ok;
    r.o[h] = ok ? (sl - b.sel.sl0) + b.sel.n * (long long)k : 0;
    cd.lo[h] = (cd.has_lo && ok) ? static_cast<const R*>(b.lo)[r.o[h]] : (R)0;
    cd.hi[h] = (cd.has_hi && ok) ? static_cast<const R*>(b.hi)[r.o[h]] : (R)0;
  }
  if (__ballot(any) == 0) return;   // (a slice none of whose elements is in the block, or owned: nothing to load)
  const int ntr = (b.fsum || b.wfsum) ? b.ntr : 0;
  const bool cw = b.cnt || b.wsum;
  if (ntr == 0) {
    walk_wm<R2, 0, true, false>(b, st, nx, cd, r, 0);
    return;
  }
  // groups of 4, 2, 1 value tracers: the most that is left; the first walk also forms cnt and wsum
  int jt = 0;
  if (cw) {
    if (ntr >= 4) { walk_wm<R2, 4, true, WF>(b, st, nx, cd, r, 0); jt = 4; }
    else if (ntr >= 2) { walk_wm<R2, 2, true, WF>(b, st, nx, cd, r, 0); jt = 2; }
    else { walk_wm<R2, 1, true, WF>(b, st, nx, cd, r, 0); jt = 1; }
  }
  for (; ntr - jt >= 4; jt += 4) walk_wm<R2, 4, false, WF>(b, st, nx, cd, r, jt);
  if (ntr - jt >= 2) { walk_wm<R2, 2, false, WF>(b, st, nx, cd, r, jt); jt += 2; }
  if (ntr - jt >= 1) walk_wm<R2, 1, false, WF>(b, st, nx, cd, r, jt);
}

// Reference layout: element (sl, column i, level k, tracer t) of f at f + sl + ld * ((i + 2) + (nx + 6) * (k + nlev * t)),
// (sl, i, k) of w at w + sl + ld * ((i + 1) + (nx + 4) * k); lo, hi at bi + n * k, cnt and wsum at bi + n * (k + nlev * c),
// fsum and wfsum at bi + n * (k + nlev * (c + 3 * r)).  x: instances of the block, y: levels.  Level nz of w is never read.
template <typename R>
__global__ void __launch_bounds__(256) ref_level_draft_kernel(const R* f, const R* w, const long long ld, const long long sl0, const long long n,
                                                             const int nx, const int nlev, const int tc, const R* lo, const R* hi,
                                                             const double wup, const double wdn, R* cnt, R* wsum, R* fsum, R* wfsum,
                                                             const int first, const int ntr) {
  const long long bi = (long long)blockIdx.x * 256 + threadIdx.x;
  if (bi >= n) return;
  const long long tstride = ld * ((long long)(nx + 6) * nlev);
  const long long nout = n * (long long)nlev;
  const int tcb = tc < 0 ? 0 : tc;
  Cond<R, 1> cd;
  cd.hasc = tc >= 0;
  cd.has_lo = lo != nullptr; cd.has_hi = hi != nullptr;
  cd.wup = (R)wup; cd.wdn = (R)wdn;
  for (long long k = blockIdx.y; k < nlev; k += gridDim.y) {
    const R* const pw = w + (sl0 + bi) + ld * ((long long)(nx + 4) * k + 2);   // column 1 of level k
    cd.top = k + 1 == nlev;
    const R* const pw1 = cd.top ? pw : pw + ld * (nx + 4);
    // column 1 of tracer tcb (f == NULL: neither compared nor summed, and the pointer is not formed)
    const R* const p = f ? f + (sl0 + bi) + ld * ((long long)(nx + 6) * (k + (long long)nlev * tcb) + 3) : pw;
    const long long o = bi + n * k;
    cd.lo[0] = cd.has_lo ? lo[o] : (R)0;
    cd.hi[0] = cd.has_hi ? hi[o] : (R)0;
    Acc<R, 1, 1> a;
    if (ntr == 0 || cnt || wsum) {
      march_draft<R, 0, true, false>(pw, pw1, p, p, 0, ld, ld, nx, cd, a);
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        if (cnt) cnt[o + nout * c] = (R)a.q[0][c];
        if (wsum) wsum[o + nout * c] = a.ws[0][c];
      }
    }
    for (int jt = 0; jt < ntr; ++jt) {
      march_draft<R, 1, false, true>(pw, pw1, p, p + tstride * (first + jt - tcb), 0, ld, ld, nx, cd, a);   // signed
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        if (fsum) fsum[o + nout * (c + (long long)NC * jt)] = a.fs[0][c][0];
        if (wfsum) wfsum[o + nout * (c + (long long)NC * jt)] = a.wf[0][c][0];
      }
    }
  }
}

bool bad_args(int ntr_all, int tc, const void* lo, const void* hi, double wup, double wdn, const void* cnt, const void* wsum,
              const void* fsum, const void* wfsum, int first, int ntr) {
  if (tc < -1 || tc >= ntr_all || (tc < 0 && (lo || hi))) return true;
  if (wup != wup || wdn != wdn || wdn > wup) return true;
  if (!cnt && !wsum && !fsum && !wfsum) return true;
  return (fsum || wfsum) && (first < 0 || ntr < 1 || first > ntr_all - ntr);
}

}  // namespace

hipError_t mpdata_level_draft_wm(const MpdataLevelDraftJob& b, hipStream_t stream) {
  WmGrid g;
  if (!b.w || bad_args(b.j.ntr, b.tc, b.lo, b.hi, b.wup, b.wdn, b.cnt, b.wsum, b.fsum, b.wfsum, b.first, b.ntr)) return hipErrorInvalidValue;
  const hipError_t e = wm_block_grid(b.j, b.sel, 1, &g);
  if (e != hipSuccess) return e;
  if (b.wfsum) return wm_block_launch(wm_level_draft_kernel<double, true>, wm_level_draft_kernel<float2, true>, b, g, stream);
  return wm_block_launch(wm_level_draft_kernel<double, false>, wm_level_draft_kernel<float2, false>, b, g, stream);
}

hipError_t mpdata_level_draft_ref(const void* f, const void* w, int elem_bytes, long long ld, long long sl0, long long n, int nx, int nlev,
                                  int ntr_all, int tc, const void* lo, const void* hi, double wup, double wdn, void* cnt, void* wsum,
                                  void* fsum, void* wfsum, int first, int ntr, hipStream_t stream) {
  if (!w || ld < 1 || sl0 < 0 || n < 1 || sl0 + n > ld || nx < 1 || nlev < 1 || ntr_all < 1) return hipErrorInvalidValue;
  if (bad_args(ntr_all, tc, lo, hi, wup, wdn, cnt, wsum, fsum, wfsum, first, ntr)) return hipErrorInvalidValue;
  if (!f && (tc >= 0 || fsum || wfsum)) return hipErrorInvalidValue;
  dim3 grid, block(256);
  if (ref_block_grid(n, nlev, &grid) != hipSuccess) return hipErrorInvalidValue;
  return ref_real(elem_bytes, [&](auto x) {
    typedef decltype(x) R;
    hipLaunchKernelGGL((ref_level_draft_kernel<R>), grid, block, 0, stream, static_cast<const R*>(f), static_cast<const R*>(w), ld, sl0, n, nx,
                       nlev, tc, static_cast<const R*>(lo), static_cast<const R*>(hi), wup, wdn, static_cast<R*>(cnt), static_cast<R*>(wsum),
                       static_cast<R*>(fsum), static_cast<R*>(wfsum), first, (fsum || wfsum) ? ntr : 0);
    return hipGetLastError();
  });
}
