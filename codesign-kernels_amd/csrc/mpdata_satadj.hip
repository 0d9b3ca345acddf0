// mpdata_satadj.hip -- saturation adjustment of a plan's tracers, in place (include/mpdata_hip.h 3y, mpdata_satadj.h): the
// condensate qn and the temperature T that goes with it, diagnosed per cell from a conserved temperature-like tracer and
// total water by a Newton iteration on the caller's saturation curves (degree-8 polynomials for liquid and ice, a linear
// ramp between them).  Pointwise in four tracers: reads two, writes one or two.  A kernel of its own outside the run:
// nothing is fused into the plan kernels, nothing is kept between calls.
//   plan layout: the walk of mpdata_wm_walk.h over the column slots 3 .. nx+2, a lane per element, as streams at signed
//     64-bit offsets from tracer th; NC columns of a lane (2 NC cells of an fp32 pair) iterate interleaved under one joint
//     exit, so that their dependent Horner chains overlap, with the next batch's loads in flight meanwhile.  No LDS, no
//     barrier; the one cross-lane operation is the __ballot that ends a wave's loop, and those that let a wave skip a
//     curve none of its cells needs (the regimes are selects by definition: skipping changes no bit).
//   reference layout: one thread per instance and level row, coalesced along sl, one loop over i.
// Built with -ffp-contract=off: every operation of the definition is rounded once, in its association; the comparisons
// are compare-and-select (NaN and -0 take the "else" value), never fmax / fmin; `/` is the correctly rounded divide.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "mpdata_satadj.h"

namespace {

using namespace wm_walk;

constexpr int NC = MPDATA_SATADJ_NC;

template <typename R> __device__ inline const MpdataSatadjPar<R>& par_of(const MpdataSatadjArgs& a);
template <> __device__ inline const MpdataSatadjPar<double>& par_of<double>(const MpdataSatadjArgs& a) { return a.par.d; }
template <> __device__ inline const MpdataSatadjPar<float>& par_of<float>(const MpdataSatadjArgs& a) { return a.par.f; }

// p, 1 / p and gz of one half of a lane's element
template <typename R>
struct Row {
  R p, rp, gz;
};

// curve(c, dc, T) of the definition for M cells at once, cell m on the row m % N: the 2 M Horner chains advance together.
// The loop over the coefficients is kept a loop: each step fetches its two coefficients with scalar loads, so that the
// 36 coefficients of the two curves need not live in scalar registers across the Newton loop (they would not fit).
template <typename R, int M, int N>
__device__ inline void curve(const R (&c)[9], const R (&dc)[9], const MpdataSatadjPar<R>& P, const Row<R> (&row)[N], const R (&T)[M],
                             R (&qs)[M], R (&dq)[M]) {
  R x[M], es[M], de[M];
#pragma unroll
  for (int m = 0; m < M; ++m) {
    x[m] = T[m] - P.t0;
    x[m] = (x[m] > P.xmin) ? x[m] : P.xmin;
    es[m] = c[8];
    de[m] = dc[8];
  }
#pragma nounroll
  for (int jj = 7; jj >= 0; --jj) {
    const R cj = c[jj], dj = dc[jj];
#pragma unroll
    for (int m = 0; m < M; ++m) {
      es[m] = cj + x[m] * es[m];
      de[m] = dj + x[m] * de[m];
    }
  }
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const R pm = row[m % N].p - es[m];
    const R den = (pm > es[m]) ? pm : es[m];
    qs[m] = (P.eps * es[m]) / den;
    dq[m] = (P.eps * de[m]) * row[m % N].rp;
  }
}

// the state of a cell, an integer in a vector register (sixteen cells' worth of lane masks would not fit the scalar ones)
enum : int { DRY = 0, DONE = 1, ACTIVE = 2 };

// sat(T) of the definition for M cells: (qs, dq, L, dL).  st[m] == ACTIVE: the cell's result is used; a wave none of whose
// cells needs a curve skips it (the values it would have given are selected away in every cell)
template <typename R, int M, int N, bool ICE>
__device__ inline void sat(const MpdataSatadjPar<R>& P, const Row<R> (&row)[N], const R (&T)[M], const int (&st)[M], R (&qs)[M],
                           R (&dq)[M], R (&L)[M], R (&dL)[M]) {
  if (!ICE) {
    curve<R, M, N>(P.esw, P.desw, P, row, T, qs, dq);
#pragma unroll
    for (int m = 0; m < M; ++m) {
      L[m] = P.lv;
      dL[m] = 0;
    }
    return;
  }
  enum : int { WARM = 0, COLD = 1, MIXED = 2 };   // (NaN: MIXED, the definition's else)
  int rg[M];
  bool nw = false, ni = false;
#pragma unroll
  for (int m = 0; m < M; ++m) {
    rg[m] = (T[m] >= P.tmax) ? WARM : (T[m] <= P.tmin) ? COLD : MIXED;
    nw = nw || (st[m] == ACTIVE && rg[m] != COLD);
    ni = ni || (st[m] == ACTIVE && rg[m] != WARM);
  }
  R qw[M], dw[M], qi[M], di[M];
#pragma unroll
  for (int m = 0; m < M; ++m) qw[m] = dw[m] = qi[m] = di[m] = 0;
  if (__ballot(nw) != 0) curve<R, M, N>(P.esw, P.desw, P, row, T, qw, dw);
  if (__ballot(ni) != 0) curve<R, M, N>(P.esi, P.desi, P, row, T, qi, di);
  const R dlm = P.an * P.lf;
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const R om = P.an * T[m] - P.bn;
    const R u = (R)1 - om;
    const R qm = om * qw[m] + u * qi[m];
    const R dm = om * dw[m] + u * di[m];
    const R lm = P.lv + u * P.lf;
    qs[m] = rg[m] == WARM ? qw[m] : rg[m] == COLD ? qi[m] : qm;
    dq[m] = rg[m] == WARM ? dw[m] : rg[m] == COLD ? di[m] : dm;
    L[m] = rg[m] == WARM ? P.lv : rg[m] == COLD ? P.ls : lm;
    dL[m] = rg[m] == MIXED ? dlm : (R)0;
  }
}

// the definition for M cells, cell m on the row m % N: h, q -> qn, T, it.  st[m]: ACTIVE where the cell's results are
// wanted (an interior column of a row that is on), else DRY: those are carried along and never iterate.  A cell stops on its own d; the
// loop ends when no cell of the wave is active.
template <typename R, int M, int N, bool ICE>
__device__ inline void satadj_cells(const MpdataSatadjPar<R>& P, const Row<R> (&row)[N], const bool hasgz, const R (&h)[M], const R (&q)[M],
                                    int (&st)[M], R (&qn)[M], R (&T)[M], int (&it)[M]) {
  R T1[M], qq[M], qs[M], dq[M], d[M], L[M], dL[M];
  bool any = false;
#pragma unroll
  for (int m = 0; m < M; ++m) {
    qq[m] = (q[m] > (R)0) ? q[m] : (R)0;
    T1[m] = hasgz ? h[m] - row[m % N].gz : h[m];
    T[m] = T1[m];
    it[m] = 0;
    d[m] = 0;
  }
  sat<R, M, N, ICE>(P, row, T, st, qs, dq, L, dL);
#pragma unroll
  for (int m = 0; m < M; ++m) {
    st[m] = (st[m] == ACTIVE && qq[m] > qs[m]) ? ACTIVE : DRY;
    any = any || st[m] == ACTIVE;
  }
  while (__ballot(any) != 0) {
    R nqs[M], ndq[M];
    sat<R, M, N, ICE>(P, row, T, st, nqs, ndq, L, dL);
    any = false;
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const R e = qq[m] - nqs[m];
      const R fff = (T1[m] - T[m]) + L[m] * e;
      const R dfff = (dL[m] * e - L[m] * ndq[m]) - (R)1;
      const R nd = (-fff) / dfff;
      const R nT = T[m] + nd;
      const bool act = st[m] == ACTIVE;
      qs[m] = act ? nqs[m] : qs[m];
      dq[m] = act ? ndq[m] : dq[m];
      d[m] = act ? nd : d[m];
      T[m] = act ? nT : T[m];
      it[m] = act ? it[m] + 1 : it[m];
      const R ad = (nd < (R)0) ? -nd : nd;   // |d| in the cell's own precision (NaN stays NaN: the cell stops)
      const bool more = ad > P.tol && it[m] < P.maxit;
      st[m] = act ? (more ? ACTIVE : DONE) : st[m];
      any = any || st[m] == ACTIVE;
    }
  }
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const R qe = qs[m] + dq[m] * d[m];
    R v = qq[m] - qe;
    v = (v > (R)0) ? v : (R)0;
    qn[m] = st[m] != DRY ? v : (R)0;
  }
}

// nx elements of a lane in four tracers: ph[0], ph[step], ... (th), the same at the offsets oq (tq), on (tn), ot (tt).  A
// half with on[h] false keeps the bits it holds in tn and tt (a lane with one half on loads them for that) and counts
// nothing; follow: the second half takes the first half's results (the phantom); a lane with no half on stores nothing.
template <typename R2, bool ICE, bool TT>
__device__ inline void march_satadj(const R2* ph, const long long oq, const long long on_, const long long ot, const long long step,
                                    const int nx, const MpdataSatadjPar<typename Elem<R2>::R>& P,
                                    const Row<typename Elem<R2>::R> (&row)[Elem<R2>::N], const bool hasgz, const bool (&on)[Elem<R2>::N],
                                    const bool follow, typename Elem<R2>::R (&cnt)[Elem<R2>::N], int (&itmax)[Elem<R2>::N]) {
  typedef Elem<R2> E;
  typedef typename E::R R;
  constexpr int N = E::N, M = NC * N;
  bool any = false, all = true;
#pragma unroll
  for (int h = 0; h < N; ++h) {
    any = any || on[h];
    all = all && on[h];
  }
  const bool keep = any && !all && !follow;   // (fp32 only) the other half of the pair keeps its bits
  const R2* const pq = ph + oq;
  R2* const pn = const_cast<R2*>(ph) + on_;
  R2* const pt = const_cast<R2*>(ph) + ot;
  R2 vh[NC], vq[NC];
#pragma unroll
  for (int u = 0; u < NC; ++u) vh[u] = ph[(long long)min(u, nx - 1) * step];
#pragma unroll
  for (int u = 0; u < NC; ++u) vq[u] = pq[(long long)min(u, nx - 1) * step];
  for (int i = 0; i < nx; i += NC) {
    R h[M], q[M], qn[M], T[M];
    int it[M], st[M];
#pragma unroll
    for (int u = 0; u < NC; ++u) {
#pragma unroll
      for (int hh = 0; hh < N; ++hh) {
        h[u * N + hh] = E::get(vh[u], hh);
        q[u * N + hh] = E::get(vq[u], hh);
        st[u * N + hh] = (on[hh] && i + u < nx) ? ACTIVE : DRY;
      }
    }
    // the next batch's loads, in flight while this one iterates (clamped duplicates of the last column are used nowhere)
    if (i + NC < nx) {
#pragma unroll
      for (int u = 0; u < NC; ++u) vh[u] = ph[(long long)min(i + NC + u, nx - 1) * step];
#pragma unroll
      for (int u = 0; u < NC; ++u) vq[u] = pq[(long long)min(i + NC + u, nx - 1) * step];
    }
    R2 kn[NC], kt[NC];
#pragma unroll
    for (int u = 0; u < NC; ++u) {
      kn[u] = R2();
      kt[u] = R2();
    }
    if (N == 2 && __ballot(keep) != 0) {
      if (keep) {
#pragma unroll
        for (int u = 0; u < NC; ++u) {
          kn[u] = pn[(long long)min(i + u, nx - 1) * step];
          if (TT) kt[u] = pt[(long long)min(i + u, nx - 1) * step];
        }
      }
    }
    satadj_cells<R, M, N, ICE>(P, row, hasgz, h, q, st, qn, T, it);
    if (any) {
#pragma unroll
      for (int u = 0; u < NC; ++u) {
        if (i + u < nx) {
          R2 sn = kn[u], st = kt[u];
#pragma unroll
          for (int hh = 0; hh < N; ++hh) {
            if (on[hh]) {
              const int m = u * N + hh;
              E::at(sn, hh) = qn[m];
              E::at(st, hh) = T[m];
              cnt[hh] = (qn[m] > (R)0) ? cnt[hh] + (R)1 : cnt[hh];
              itmax[hh] = (it[m] > itmax[hh]) ? it[m] : itmax[hh];
            }
          }
          if (N == 2 && follow) {
            E::at(sn, N - 1) = E::get(sn, 0);
            E::at(st, N - 1) = E::get(st, 0);
          }
          pn[(long long)(i + u) * step] = sn;
          if (TT) pt[(long long)(i + u) * step] = st;
        }
      }
    }
  }
}

// Plan layout: a wave per (tile of the block, 64-element slice of the chunk), lane -> element e = s * nlev + kk.
// R2: one 8-byte element (double, or the float2 of two adjacent slots).
template <typename R2, bool ICE, bool TT>
__global__ void __launch_bounds__(256) wm_satadj_kernel(const MpdataSatadjJob b, const long long t0, const int ntile, const int nslice) {
  typedef Elem<R2> E;
  typedef typename E::R R;
  const MpdataLayoutJob& j = b.j;
  const MpdataSatadjArgs& a = b.a;
  const MpdataSatadjPar<R>& P = par_of<R>(a);
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
  const R2* ph = static_cast<const R2*>(j.prv) + (long long)a.th * j.prv_tstride + tile * j.prv_tile_stride +
                 (in_main ? e : (long long)j.ncol_p * j.main_e + (e - j.main_e)) + 3 * cstep;   // column 1 = slot 3
  // signed: a tracer below th walks back
  const long long oq = (long long)(a.tq - a.th) * j.prv_tstride, on_ = (long long)(a.tn - a.th) * j.prv_tstride;
  const long long ot = TT ? (long long)(a.tt - a.th) * j.prv_tstride : on_;
  // per half: the instance and the tall level the slot stands for, its row and its place in the outputs
  const int nzm = b.sel.nz - 1;
  const long long nslots = b.sel.ncrms * b.sel.W;   // slots that are an instance (a window of one)
  Row<R> row[E::N];
  bool in[E::N], on[E::N];
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
    in[h] = ok;
    o[h] = ok ? (sl - b.sel.sl0) + b.sel.n * (long long)k : 0;
    row[h].p = ok ? static_cast<const R*>(a.pres)[o[h]] : (R)0;
    on[h] = ok && row[h].p != (R)0;
    row[h].rp = on[h] ? (R)1 / row[h].p : (R)0;
    row[h].gz = (a.gz && ok) ? static_cast<const R*>(a.gz)[o[h]] : (R)0;
  }
  // the phantom half of an odd fp32 plan follows the plan's last slot, its partner in the element (W > 1: the caller
  // restores the inner plan's phantom behind the kernel)
  const bool follow = E::N == 2 && b.sel.W == 1 && (nslots & 1) && act && (tile * j.slp + s) * E::N + 1 == nslots && on[0];
  bool any = false;
#pragma unroll
  for (int h = 0; h < E::N; ++h) any = any || on[h];
  R cnt[E::N];
  int itmax[E::N];
#pragma unroll
  for (int h = 0; h < E::N; ++h) {
    cnt[h] = 0;
    itmax[h] = 0;
  }
  // (a slice whose elements all lie outside the block or have pres == 0: nothing to load)
  if (__ballot(any) != 0) march_satadj<R2, ICE, TT>(ph, oq, on_, ot, cstep, nx, P, row, a.gz != nullptr, on, follow, cnt, itmax);
#pragma unroll
  for (int h = 0; h < E::N; ++h) {
    if (in[h]) {
      if (a.ncld) static_cast<R*>(a.ncld)[o[h]] = cnt[h];
      if (a.iters) static_cast<R*>(a.iters)[o[h]] = (R)itmax[h];
    }
  }
}

// Reference layout: element (sl, column i, level k, tracer t) at f + sl + ld * ((i + 2) + (nx + 6) * (k + nlev * t));
// pres, gz, ncld, iters at bi + n * k.  x: instances of the block, y: levels.
template <typename R, bool ICE>
__global__ void __launch_bounds__(256) ref_satadj_kernel(R* f, const long long ld, const long long sl0, const long long n, const int nx,
                                                        const int nlev, const MpdataSatadjArgs a) {
  const MpdataSatadjPar<R>& P = par_of<R>(a);
  const long long bi = (long long)blockIdx.x * 256 + threadIdx.x;
  if (bi >= n) return;
  const long long ts = ld * ((long long)(nx + 6) * nlev);   // tracer stride
  const long long oq = ts * (a.tq - a.th), on_ = ts * (a.tn - a.th), ot = a.tt >= 0 ? ts * (a.tt - a.th) : on_;   // signed
  for (long long k = blockIdx.y; k < nlev; k += gridDim.y) {
    const R* const p = f + (sl0 + bi) + ld * ((long long)(nx + 6) * (k + (long long)nlev * a.th) + 3);   // column 1 of tracer th
    const long long o = bi + n * k;
    Row<R> row[1];
    row[0].p = static_cast<const R*>(a.pres)[o];
    row[0].gz = a.gz ? static_cast<const R*>(a.gz)[o] : (R)0;
    R cnt = 0;
    int itmax = 0;
    if (row[0].p != (R)0) {
      row[0].rp = (R)1 / row[0].p;
      for (int i = 0; i < nx; ++i) {
        const R h[1] = {p[i * ld]}, q[1] = {p[i * ld + oq]};
        R qn[1], T[1];
        int it[1], st[1] = {ACTIVE};
        satadj_cells<R, 1, 1, ICE>(P, row, a.gz != nullptr, h, q, st, qn, T, it);
        const_cast<R*>(p)[i * ld + on_] = qn[0];
        if (a.tt >= 0) const_cast<R*>(p)[i * ld + ot] = T[0];
        cnt = (qn[0] > (R)0) ? cnt + (R)1 : cnt;
        itmax = (it[0] > itmax) ? it[0] : itmax;
      }
    }
    if (a.ncld) static_cast<R*>(a.ncld)[o] = cnt;
    if (a.iters) static_cast<R*>(a.iters)[o] = (R)itmax;
  }
}

bool tracers_ok(const MpdataSatadjArgs& a, const int ntr) {
  const int t[4] = {a.th, a.tq, a.tn, a.tt};
  for (int x = 0; x < 4; ++x) {
    if (t[x] >= ntr || t[x] < (x == 3 ? -1 : 0)) return false;
    for (int y = 0; y < x; ++y)
      if (t[x] >= 0 && t[x] == t[y]) return false;
  }
  return a.pres != nullptr;
}

}  // namespace

hipError_t mpdata_satadj_wm(const MpdataSatadjJob& b, hipStream_t stream) {
  WmGrid g;
  if (!tracers_ok(b.a, b.j.ntr)) return hipErrorInvalidValue;
  const hipError_t e = wm_block_grid(b.j, b.sel, 1, &g);
  if (e != hipSuccess) return e;
  const bool ice = b.a.ice != 0, tt = b.a.tt >= 0;
  if (ice && tt) return wm_block_launch(wm_satadj_kernel<double, true, true>, wm_satadj_kernel<float2, true, true>, b, g, stream);
  if (ice) return wm_block_launch(wm_satadj_kernel<double, true, false>, wm_satadj_kernel<float2, true, false>, b, g, stream);
  if (tt) return wm_block_launch(wm_satadj_kernel<double, false, true>, wm_satadj_kernel<float2, false, true>, b, g, stream);
  return wm_block_launch(wm_satadj_kernel<double, false, false>, wm_satadj_kernel<float2, false, false>, b, g, stream);
}

hipError_t mpdata_satadj_ref(void* f, int elem_bytes, long long ld, long long sl0, long long n, int nx, int nlev, int ntr,
                             const MpdataSatadjArgs& a, hipStream_t stream) {
  if (!f || ld < 1 || sl0 < 0 || n < 1 || sl0 + n > ld || nx < 1 || nlev < 1 || !tracers_ok(a, ntr)) return hipErrorInvalidValue;
  dim3 grid, block(256);
  if (ref_block_grid(n, nlev, &grid) != hipSuccess) return hipErrorInvalidValue;
  return ref_real(elem_bytes, [&](auto x) {
    typedef decltype(x) R;
    if (a.ice) hipLaunchKernelGGL((ref_satadj_kernel<R, true>), grid, block, 0, stream, static_cast<R*>(f), ld, sl0, n, nx, nlev, a);
    else hipLaunchKernelGGL((ref_satadj_kernel<R, false>), grid, block, 0, stream, static_cast<R*>(f), ld, sl0, n, nx, nlev, a);
    return hipGetLastError();
  });
}
