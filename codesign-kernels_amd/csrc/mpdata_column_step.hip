// mpdata_column_step.hip -- the fused column step of f, in place (include/mpdata_hip.h 3q, mpdata_column_step.h): per-cell
// source, large-scale vertical advection, sedimentation and the implicit vertical solve of one column in one call, with
// one read of f and one write.  Kernels of their own outside the run: nothing is fused into the plan kernels, nothing is
// kept between calls.
//   plan layout: the geometry and the copy stage of mpdata_vsolve.hip.  A workgroup takes UG adjacent units (8-byte
//     elements of the instance axis) and CB columns: its four waves copy the column slots of the group's tiles as linear
//     streams into LDS, re-laid as [column][unit][level] with an odd level stride; after a barrier a lane per (unit, column) sweeps its column in LDS in place through the present
//     stages; after a second barrier the waves store LDS back to f as the same linear streams.  s, wp and the coefficient
//     rows cb, cc, ir, lo, p, g are read by the sweeping lanes from the caller's arrays, the unit fastest (16 units of a row are
//     one 128-byte line, the same line for every column of the batch), LA levels ahead of the chain.
//     Race freedom: workgroups own disjoint (group, column batch) element sets; every global load of f
//     precedes the first barrier and every global store of f follows the second; between them a lane touches only its own
//     column in LDS; idle lanes clamp their addresses and store nothing; no barrier sits under a condition that differs
//     inside a workgroup.
//   reference layout: one thread per instance, coalesced along sl, rows (column, tracer) over grid.y; the thread owns its
//     column and sweeps it in place in device memory.
// The set of present stages is a template argument: an absent stage costs nothing.
// Built with -ffp-contract=off and IEEE divides: every operation of the definition is rounded once, in its association.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "mpdata_column_step.h"

namespace {

using namespace wm_walk;

// (LDS_ELEMS, the LDS of a workgroup at most, and the column groups of the launch: mpdata_wm_walk.h)
constexpr int LA = 3;             // levels of operands read ahead of the chain
enum { SRC = 1, SUB = 2, SED = 4, VS = 8 };   // the stages of a kernel's template argument

__device__ inline double pos(double a) { return fmax(a, 0.0); }
__device__ inline float pos(float a) { return fmaxf(a, 0.0f); }

// what the sweeping lanes read of the caller's arrays, typed (NULL: the stage is absent from the kernel)
template <typename R>
struct Coef {
  const R *s, *cb, *cc, *wp, *lo, *p, *g;
  const R* ir;   // plan layout: 1 / (rho * adz) (n, nlev) from wm_ir_kernel; reference layout: NULL, formed by the thread
  R* psfc;
  R cf;   // c, rounded once
  int clip;
  long long n;
};
// The plan-layout kernel sends the nine array addresses of its argument through LDS once -- one thread writes them in
// front of the copy stage, every sweeping lane reads them back behind the first barrier -- so that they are dead while the
// copy stage runs and the sweeps hold them in vector registers: held by the scalar unit from the kernel's entry to the
// sweeps, beside the geometry of the copy stage, they are more than the scalar registers a kernel has.
constexpr int NPAR = 9;
template <typename R>
__device__ inline void par_put(unsigned long long* const lp, const Coef<R>& q) {
  lp[0] = (unsigned long long)q.s; lp[1] = (unsigned long long)q.cb; lp[2] = (unsigned long long)q.cc; lp[3] = (unsigned long long)q.wp;
  lp[4] = (unsigned long long)q.lo; lp[5] = (unsigned long long)q.p; lp[6] = (unsigned long long)q.g; lp[7] = (unsigned long long)q.ir;
  lp[8] = (unsigned long long)q.psfc;
}
template <typename R>
__device__ inline Coef<R> par_get(const unsigned long long* const lp, Coef<R> q) {
  q.s = (const R*)lp[0]; q.cb = (const R*)lp[1]; q.cc = (const R*)lp[2]; q.wp = (const R*)lp[3];
  q.lo = (const R*)lp[4]; q.p = (const R*)lp[5]; q.g = (const R*)lp[6]; q.ir = (const R*)lp[7];
  q.psfc = (R*)lp[8];
  return q;
}
template <typename R>
Coef<R> coef(const MpdataColumnStepArrays& a, const long long n, const int nlev) {
  Coef<R> q;
  q.s = static_cast<const R*>(a.s); q.cb = static_cast<const R*>(a.cb); q.cc = static_cast<const R*>(a.cc);
  q.wp = static_cast<const R*>(a.wp); q.lo = static_cast<const R*>(a.lo); q.p = static_cast<const R*>(a.pg);
  q.g = a.pg ? q.p + n * nlev : nullptr;
  q.psfc = static_cast<R*>(a.psfc);
  q.ir = nullptr;
  q.cf = (R)a.c; q.clip = a.clip; q.n = n;
  return q;
}

// The sweeps of one lane over the nlev levels of its column pf[0], pf[fs], ..., the N halves of an element in lockstep.
//   bi[h]: the instance of half h in the block (clamped to 0 where the half is not on); on[h]: the half is written, else
//   it keeps what it held;  cell0: the offset of (column, level 1, tracer) in s and wp, lstep their level stride; poff the
//   offset of (column, tracer) in psfc;  irf(k): 1 / (rho * adz) of level k, per half.
// Upward pass, level k per step: gn = source(f(k+1)) is read BEFORE level k or k - 1 is written; v = subside(gm, gc, gn) is
// level k after stage 2; sedimentation finishes level k - 1 from the carried prev = v(k-1), fzc = Fz(k-1) and Fz(k) = wp(k)
// * v; the forward sweep takes each finished level with y(k-1) carried in cy (y(1) through the general statement with a
// carried +0 and lo = +0, as mpdata_vsolve.h argues).  Downward pass: x over y with x(k+1) carried, g(nlev) = +0.
template <typename R2, int ST, typename FS, typename IR>
__device__ inline void column_sweeps(R2* const pf, const FS fs, const int nlev, const Coef<typename Elem<R2>::R>& q,
                                     const long long (&bi)[Elem<R2>::N], const bool (&on)[Elem<R2>::N], const long long cell0,
                                     const long long lstep, const long long poff, const IR irf) {
  typedef Elem<R2> E;
  typedef typename E::R R;
  constexpr int N = E::N;
  constexpr bool src = (ST & SRC) != 0, sub = (ST & SUB) != 0, sed = (ST & SED) != 0, vs = (ST & VS) != 0;
  const long long n = q.n;
  auto source =[&](const R fv, const R sv) -> R {
    if (!src) return fv;
    const R pr = q.cf * sv;
    R gv = fv + pr;
    if (q.clip) gv = pos(gv);
    return gv;
  };
  R cy[N];
  auto emit = [&](const int ke, const int h, R v, const R lov, const R pv) {
    if (vs) {
      const R m = lov * cy[h];
      const R r = v - m;
      cy[h] = r * pv;
      v = cy[h];
    }
    if (on[h]) E::at(pf[ke * fs], h) = v;
  };
  R gm[N], gc[N], prev[N], fzc[N];
#pragma unroll
  for (int h = 0; h < N; ++h) { cy[h] = 0; gm[h] = 0; gc[h] = 0; prev[h] = 0; fzc[h] = 0; }
  if (sub) {
    const R2 f0 = pf[0];
#pragma unroll
    for (int h = 0; h < N; ++h) {
      gc[h] = source(E::get(f0, h), src ? q.s[bi[h] + cell0] : (R)0);
      gm[h] = gc[h];   // kb = max(1, k - 1): the level itself
    }
  }
  for (int kb = 0; kb < nlev; kb += LA) {
    R2 fv[LA], irv[LA];
    R sv[LA][N], cbv[LA][N], ccv[LA][N], wpv[LA][N], lov[LA][N], pv[LA][N];
#pragma unroll
    for (int u = 0; u < LA; ++u) {
      const int k = min(kb + u, nlev - 1);
      const int kf = sub ? min(k + 1, nlev - 1) : k;   // the level read of f and s
      const int ke = sed ? max(k - 1, 0) : k;          // the level finished in this step
      fv[u] = pf[kf * fs];
      irv[u] = fv[u];
      if (sed) irv[u] = irf(ke);
#pragma unroll
      for (int h = 0; h < N; ++h) {
        const long long o = bi[h] + n * k, oe = bi[h] + n * ke;
        sv[u][h] = src ? q.s[bi[h] + cell0 + lstep * kf] : (R)0;
        cbv[u][h] = sub ? q.cb[o] : (R)0;
        ccv[u][h] = sub ? q.cc[o] : (R)0;
        wpv[u][h] = sed ? q.wp[bi[h] + cell0 + lstep * k] : (R)0;
        lov[u][h] = vs && ke > 0 ? q.lo[oe] : (R)0;   // (lo of level 1 is never read)
        pv[u][h] = vs ? q.p[oe] : (R)0;
      }
    }
#pragma unroll
    for (int u = 0; u < LA; ++u) {
      if (kb + u < nlev) {
        const int k = kb + u;
#pragma unroll
        for (int h = 0; h < N; ++h) {
          R v;
          if (sub) {
            const R gn = k + 1 < nlev ? source(E::get(fv[u], h), sv[u][h]) : gc[h];   // kc = min(nlev, k + 1)
            const R a = gc[h] - gm[h], c = gn - gc[h];
            const R pa = cbv[u][h] * a, pc = ccv[u][h] * c;
            const R dec = pa + pc;
            v = gc[h] - dec;
            gm[h] = gc[h];
            gc[h] = gn;
          } else {
            v = source(E::get(fv[u], h), sv[u][h]);
          }
          if (sed) {
            const R fz = wpv[u][h] * v;
            if (k > 0) {
              const R d = fzc[h] - fz;
              const R dec = d * E::get(irv[u], h);
              emit(k - 1, h, prev[h] - dec, lov[u][h], pv[u][h]);
            } else if (q.psfc && on[h]) {
              q.psfc[bi[h] + poff] = fz;   // Fz(i,1) of the field that enters the stage
            }
            prev[h] = v;
            fzc[h] = fz;
          } else {
            emit(k, h, v, lov[u][h], pv[u][h]);
          }
        }
      }
    }
  }
  if (sed) {   // the top level: Fz(nlev + 1) = +0
    const R2 irt = irf(nlev - 1);
#pragma unroll
    for (int h = 0; h < N; ++h) {
      const long long oe = bi[h] + n * (nlev - 1);
      const R lot = vs && nlev > 1 ? q.lo[oe] : (R)0, pt = vs ? q.p[oe] : (R)0;
      const R d = fzc[h] - (R)0;
      const R dec = d * E::get(irt, h);
      emit(nlev - 1, h, prev[h] - dec, lot, pt);
    }
  }
  if (vs) {
#pragma unroll
    for (int h = 0; h < N; ++h) cy[h] = 0;
    for (int kb = 0; kb < nlev; kb += LA) {
      R2 yv[LA];
      R gv[LA][N];
#pragma unroll
      for (int u = 0; u < LA; ++u) {
        const int k = nlev - 1 - min(kb + u, nlev - 1);
        yv[u] = pf[k * fs];
#pragma unroll
        for (int h = 0; h < N; ++h) gv[u][h] = q.g[bi[h] + n * k];
      }
#pragma unroll
      for (int u = 0; u < LA; ++u) {
        if (kb + u < nlev) {
          const int k = nlev - 1 - kb - u;
#pragma unroll
          for (int h = 0; h < N; ++h) {
            const R m = gv[u][h] * cy[h];
            cy[h] = E::get(yv[u], h) - m;
            if (on[h]) E::at(pf[k * fs], h) = cy[h];
          }
        }
      }
    }
  }
}

// The workgroups of the plan-layout kernel, as in mpdata_vsolve.hip.  A UNIT is one 8-byte element of the instance axis
// (an instance, or the pair 2 * ue, 2 * ue + 1 of an fp32 plan): slot ue % slp of tile ue / slp.  A workgroup takes UG
// adjacent units (a multiple of slp) and CB adjacent columns.
template <typename R>
struct CsArgs {
  void* f;                    // the plan side of f, first tracer of the call
  Coef<R> q;
  long long sl0, ncrms;
  long long tstride, tile_stride;
  int t0, t1;                 // tiles the block touches
  int g0, ngroup;             // first group, groups
  int chunk, main_e, ncol_p, nlev, slp;
  int UG, CB, ncb, ns;        // ns: level stride in LDS (odd)
  int ush;                    // UG = 1 << ush
};

// Plan layout.  blockIdx.x = (tracer * ngroup + group) * ncb + column batch; R2: one 8-byte element (double, or the float2
// of two adjacent slots); ST: the present stages.
template <typename R2, int ST>
__global__ void __launch_bounds__(256) wm_column_step_kernel(const CsArgs<typename Elem<R2>::R> g) {
  typedef Elem<R2> E;
  typedef typename E::R R;
  constexpr int N = E::N;
  extern __shared__ __align__(8) unsigned char cs_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int bx = blockIdx.x;
  const int cb = bx % g.ncb;
  bx /= g.ncb;
  const int gi = bx % g.ngroup;
  const int tr = bx / g.ngroup;
  const int nlev = g.nlev, nx = g.ncol_p - 6, slp = g.slp, ns = g.ns, UG = g.UG;
  const long long n = g.q.n, sl0 = g.sl0;
  const int c0 = cb * g.CB, cbn = min(g.CB, nx - c0);
  const int ue0 = (g.g0 + gi) * UG;
  const int tile0 = ue0 / slp, ntg = UG / slp;
  const int nslice = (g.chunk + 63) / 64;
  const int rem_e = g.chunk - g.main_e;
  R2* const lf = reinterpret_cast<R2*>(cs_lds);   // [column][unit][ns]: f, in place through the stages
  unsigned long long* const lpar = reinterpret_cast<unsigned long long*>(lf + g.CB * UG * ns);   // [NPAR]: the array addresses
  R2* const f = static_cast<R2*>(g.f) + (long long)tr * g.tstride;
  const int ci = tid >> g.ush, ug = tid & (UG - 1);   // the lane's pair in the sweeps
  const bool act = ci < cbn;
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
  if (tid == 0) par_put(lpar, g.q);
  copy(false);
  __syncthreads();
  // ---- the sweeps: a lane per (unit, column)
  if (act) {
    bool on[N], any = false;
    long long bi[N];
#pragma unroll
    for (int h = 0; h < N; ++h) {
      const long long sl = (long long)ue * N + h;
      on[h] = sl >= sl0 && sl < sl0 + n;
      bi[h] = on[h] ? sl - sl0 : 0;   // (a half that is not on reads the block's first instance and stores nothing)
      any = any || on[h];
    }
    if (any) {
      R2* const pf = lf + ((long long)ci * UG + ug) * ns;
      const long long col = c0 + ci;
      const Coef<R> q = par_get(lpar, g.q);
      const R* const gir = q.ir;
      column_sweeps<R2, ST>(pf, 1, nlev, q, bi, on, n * (col + (long long)nx * nlev * tr), n * nx, n * (col + (long long)nx * tr),
                            [&](const int k) {
                              R2 v;
#pragma unroll
                              for (int h = 0; h < N; ++h) E::at(v, h) = gir[bi[h] + n * k];
                              return v;
                            });
      // the phantom half follows the plan's last instance, its partner in the pair
      if (N == 2 && (g.ncrms & 1) && (long long)ue * N + 1 == g.ncrms && on[0]) {
        for (int k = 0; k < nlev; ++k) {
          R2 v = pf[k];
          E::at(v, N - 1) = E::get(v, 0);
          pf[k] = v;
        }
      }
    }
  }
  __syncthreads();
  copy(true);
}

// 1 / (rho * adz) of the block's instances from the plan's kc array ([tile][rho, adz, rhow][slot][level], 8-byte elements)
// into ir (n, nlev), leading dimension n: one rounded multiply, one IEEE divide.  x: instances of the block, y: levels.  A
// small kernel IN FRONT of the sweeps, as the factors of stage 4: the divides stay out of the hot kernel, and its lanes
// read ir as they read the coefficient rows.
template <typename R2>
__global__ void __launch_bounds__(256) wm_ir_kernel(const R2* __restrict__ rho, const R2* __restrict__ adz, const long long kc_tile_stride,
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
// and adz at sl + ld * (k - 1).  x: instances of the block, y: rows r = (i - 1) + nx * t.
template <typename R, int ST>
__global__ void __launch_bounds__(256) ref_column_step_kernel(R* f, const R* __restrict__ rho, const R* __restrict__ adz, const Coef<R> q,
                                                             const long long ld, const long long sl0, const int nx, const int nlev,
                                                             const long long rows) {
  const long long b0 = (long long)blockIdx.x * 256 + threadIdx.x;
  if (b0 >= q.n) return;
  const long long sl = sl0 + b0, step = ld * (nx + 6);
  const long long bi[1] = {b0};
  const bool on[1] = {true};
  for (long long r = blockIdx.y; r < rows; r += gridDim.y) {
    const long long t = r / nx, i = r - t * nx;
    R* const pf = f + sl + ld * ((i + 3) + (long long)(nx + 6) * nlev * t);
    column_sweeps<R, ST>(pf, step, nlev, q, bi, on, q.n * (i + (long long)nx * nlev * t), q.n * nx, q.n * r,
                         [&](const int k) { return (R)1 / (rho[sl + ld * k] * adz[sl + ld * k]); });
  }
}

// the kernels by their set of stages (1 .. 15)
#define MPD_CS_CASES K(1) K(2) K(3) K(4) K(5) K(6) K(7) K(8) K(9) K(10) K(11) K(12) K(13) K(14) K(15)
template <typename R2>
void (*wm_kernel(const int st))(CsArgs<typename Elem<R2>::R>) {
  switch (st) {
#define K(x) case x: return wm_column_step_kernel<R2, x>;
    MPD_CS_CASES
#undef K
  }
  return nullptr;
}
template <typename R>
void (*ref_kernel(const int st))(R*, const R*, const R*, Coef<R>, long long, long long, int, int, long long) {
  switch (st) {
#define K(x) case x: return ref_column_step_kernel<R, x>;
    MPD_CS_CASES
#undef K
  }
  return nullptr;
}

// the stages of a call; 0: none, -1: half a stage, or psfc without wp
int stages_of(const MpdataColumnStepArrays& a) {
  if (!a.cb != !a.cc || !a.lo != !a.pg || (a.psfc && !a.wp)) return -1;
  return (a.s ? SRC : 0) | (a.cb ? SUB : 0) | (a.wp ? SED : 0) | (a.lo ? VS : 0);
}

template <typename R2>
hipError_t wm_launch(const MpdataColumnStepJob& b, const WmGrid& wg, const int st, hipStream_t stream) {
  typedef typename Elem<R2>::R R;
  const MpdataLayoutJob& j = b.j;
  const int slp = j.slp;
  CsArgs<R> g;
  g.f = j.prv;
  g.q = coef<R>(b.a, b.sel.n, j.nlev);
  g.q.ir = static_cast<const R*>(b.ir);
  g.sl0 = b.sel.sl0; g.ncrms = b.sel.ncrms;
  g.tstride = j.prv_tstride; g.tile_stride = j.prv_tile_stride;
  g.t0 = (int)wg.t0; g.t1 = (int)(wg.t0 + wg.ntile - 1);
  g.chunk = (int)j.chunk; g.main_e = (int)j.main_e; g.ncol_p = j.ncol_p; g.nlev = j.nlev; g.slp = slp;
  // the columns and the array addresses alone: the coefficients are read where they lie
  ColGroups cg;
  if (j.chunk > 2147483647LL || j.main_e > 2147483647LL ||
      !col_groups_batched(j, b.sel, wg, LDS_ELEMS, /*fixed*/ NPAR, /*rows*/ 0, /*unit_mul*/ 1, &cg))
    return hipErrorInvalidValue;
  col_groups_fill(cg, &g);
  g.ncb = cg.ncb; g.ush = cg.ush;
  const unsigned blocks = (unsigned)(cg.ngroup * j.ntr * g.ncb);
  const size_t lds = (size_t)cg.lds_e * 8;
  if (st & SED) {
    dim3 grid;
    if (ref_block_grid(b.sel.n, j.nlev, &grid) != hipSuccess) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wm_ir_kernel<R2>, grid, dim3(256), 0, stream, static_cast<const R2*>(b.rho), static_cast<const R2*>(b.adz),
                       b.kc_tile_stride, b.sel.sl0, b.sel.n, slp, j.nlev, static_cast<R*>(b.ir));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(wm_kernel<R2>(st), dim3(blocks), dim3(256), lds, stream, g);
  return hipGetLastError();
}

}  // namespace

hipError_t mpdata_column_step_wm(const MpdataColumnStepJob& b, hipStream_t stream) {
  WmGrid wg;
  const MpdataLayoutJob& j = b.j;
  const int st = stages_of(b.a);
  if (st < 1 || b.sel.W != 1 || j.prv_col0 != 0 || j.ncols != j.ncol_p) return hipErrorInvalidValue;
  if ((st & SED) && (!b.rho || !b.adz || !b.ir || b.kc_tile_stride < j.chunk)) return hipErrorInvalidValue;
  const hipError_t e = wm_block_grid(j, b.sel, j.ntr, &wg);
  if (e != hipSuccess) return e;
  return b.sel.ipe == 1 ? wm_launch<double>(b, wg, st, stream) : wm_launch<float2>(b, wg, st, stream);
}

hipError_t mpdata_column_step_ref(void* f, const void* rho, const void* adz, int elem_bytes, long long ld, long long sl0, long long n,
                                  int nx, int nlev, int ntr, const MpdataColumnStepArrays& a, hipStream_t stream) {
  const int st = stages_of(a);
  if (!f || st < 1 || ld < 1 || sl0 < 0 || n < 1 || sl0 + n > ld || nx < 1 || nlev < 1 || ntr < 1 || (elem_bytes != 4 && elem_bytes != 8))
    return hipErrorInvalidValue;
  if ((st & SED) && (!rho || !adz)) return hipErrorInvalidValue;
  const long long rows = (long long)nx * ntr;
  dim3 grid;
  if (ref_block_grid(n, rows, &grid) != hipSuccess) return hipErrorInvalidValue;
  return ref_real(elem_bytes, [&](auto r) {
    typedef decltype(r) R;
    hipLaunchKernelGGL(ref_kernel<R>(st), grid, dim3(256), 0, stream, static_cast<R*>(f), static_cast<const R*>(rho),
                       static_cast<const R*>(adz), coef<R>(a, n, nlev), ld, sl0, nx, nlev, rows);
    return hipGetLastError();
  });
}
