// mpdata_column_cond.hip -- per-column conditional level counts, bottoms, tops and mass-weighted paths of the tracers of f
// under a condition on one of them, and their reductions over the columns (include/mpdata_hip.h 3w, mpdata_column_cond.h):
// the second block call that reduces along the LEVELS, in a kernel of its own outside the run (nothing is fused into the
// plan kernels, nothing is kept between calls).
//   plan layout: the staging of mpdata_column_path.hip -- a workgroup copies the column slots of a group of adjacent
//     units and a batch of columns through LDS as linear streams, re-laid as [column][unit][level] with an odd level
//     stride, next to three coefficient rows [unit][level]: rho * adz, lo and hi of the group's slots.  The condition
//     tracer is staged first; a lane per (unit, column) walks its levels in rising order, counts, and keeps the in-bits
//     in CC_MW 32-bit registers per half.  The value tracers follow through the same columns of LDS, each summed under
//     the bits.  Register arrays are read and written at compile-time positions only (rotate_in): no
//     run-time register index, no scratch.
//   reference layout: one thread per (instance, column), coalesced along sl, the loops over k and the tracers inside.
// Built with -ffp-contract=off: every operation of the definition is rounded once, in the definition's association.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "mpdata_column_cond.h"

namespace {

using namespace wm_walk;

// 8-byte elements of LDS per workgroup: LDS_ELEMS of mpdata_wm_walk.h (40 KiB, four workgroups per CU).  With three rows
// next to the columns the 32 KiB of mpdata_column_path.hip left 6 columns a batch at 28 levels and ONE at 63 (a window),
// and every batch stages the rows again: 17 % to 22 % slower on plain plans, 84 % to 90 % on windowed ones
// (docs/EXPERIMENTS.md AG; -DMPDATA_COLUMN_COND_LDS_ELEMS=4096 builds that form to time against).
#ifndef MPDATA_COLUMN_COND_LDS_ELEMS
#define MPDATA_COLUMN_COND_LDS_ELEMS LDS_ELEMS
#endif
constexpr int CC_LDS_ELEMS = MPDATA_COLUMN_COND_LDS_ELEMS;
constexpr int CC_MW = 8;             // 32-bit words of in-bits per half: 256 levels of a plan
constexpr int CC_MW_WIN = 2;         // ... 64 levels of a window
constexpr int CC_TCH = 8;            // windowed plans: value tracers summed under one staging of the condition

struct CcGeom {
  long long t0, t1;   // tiles the block touches
  long long g0;       // first group
  long long ngroup;
  int UG, CB, ncb, ns;   // ns: level stride in LDS (odd)
};
// the kernel's arguments as they lie at the start of its LDS, and their size in 8-byte elements (the `fixed` elements of
// col_groups_batched, with the window table behind the rows)
struct CcArgs {
  MpdataColumnCondJob b;
  CcGeom g;
};
constexpr int CC_ARGS_E = (int)((sizeof(CcArgs) + 7) / 8);

// a[0 .. N-2] = a[1 .. N-1], a[N-1] = v: the words of the in-bits (and the running sums of a windowed plan's tracers) pass
// through a[0] one after the other, so that a loop over them that is NOT unrolled still reads and writes a register at a
// compile-time position; N steps bring every element home
template <int X, typename T, int N>
__device__ __forceinline__ void rotate_from(T (&a)[N], const T v) {
  if constexpr (X + 1 < N) {
    a[X] = a[X + 1];
    rotate_from<X + 1>(a, v);
  } else {
    a[X] = v;
  }
}
template <typename T, int N>
__device__ __forceinline__ void rotate_in(T (&a)[N], const T v) {
  rotate_from<0>(a, v);
}

// the levels [lo, hi) of its chunk slot that a slot adds to instance *sl, level kk of them the tall level *k0 + kk + 1:
// all of them, of a window the owned ones; none for padding, the phantom, the partner of a split pair and neighbours in
// the group.  The slot: half h of unit ue (W = 1: x = h), or slot x = m * N + h of the N * W slots of unit ue of a
// windowed plan -- window x mod W of instance ue * N + x / W; wt: the window table in LDS, (k0, lo, hi, -) per window.
template <bool WIN>
__device__ inline void slot_levels(const MpdataBlockSel& sel, const int* wt, const int nlev, const long long ue, const int N, const int x,
                                   long long* sl, int* k0, int* lo, int* hi) {
  *sl = ue * N + x; *k0 = 0; *lo = 0; *hi = nlev;
  if (WIN) {
    const int d = x >= sel.W ? 1 : 0, win = x - d * sel.W;   // (x < N * W, N <= 2)
    *sl = ue * N + d;
    *k0 = wt[4 * win]; *lo = wt[4 * win + 1]; *hi = wt[4 * win + 2];
  }
  if (*sl < sel.sl0 || *sl >= sel.sl0 + sel.n) *hi = *lo = 0;
}

// Plan layout.  blockIdx.x = group * ncb + column batch; R2: one 8-byte element; WIN: a windowed plan (W > 1); HL, HH: lo,
// hi are given (compile-time, so that the level loops hold no flag and no mask for an absent bound).
template <typename R2, bool WIN, bool HL, bool HH>
__global__ void __launch_bounds__(256) wm_column_cond_kernel(const MpdataColumnCondJob ba, const CcGeom ga) {
  typedef Elem<R2> E;
  typedef typename E::R R;
  extern __shared__ __align__(8) unsigned char cc_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // The arguments go through LDS once: held in scalar registers across the window / tracer / level nest, the addresses,
  // the 64-bit strides and the block overflowed them (dozens of scalar spills).  From here on `b` and `g` are the copies
  // in LDS, read where they are used; what steers the uniform control flow -- the counts below, the
  // number of value tracers -- is taken from the arguments themselves and stays scalar.
  CcArgs* const sa = reinterpret_cast<CcArgs*>(cc_lds);
  if (tid == 0) { sa->b = ba; sa->g = ga; }
  __syncthreads();
  const MpdataColumnCondJob& b = sa->b;
  const CcGeom& g = sa->g;
  const MpdataLayoutJob& j = b.j;
  const long long bx = blockIdx.x;
  const int cb = (int)(bx % ga.ncb);
  const long long gi = bx / ga.ncb;
  const int nlev = ba.j.nlev, nx = ba.j.ncol_p - 6, slp = ba.j.slp, W = WIN ? ba.sel.W : 1, ns = ga.ns, UG = ga.UG;
  const int c0 = cb * ga.CB, cbn = min(ga.CB, nx - c0);
  // (what the launcher has checked, told to the compiler: no loop of the nest needs a guard for an empty trip, which would
  // be one more mask held in scalar registers across it)
  __builtin_assume(nlev >= 1 && nlev <= 256 && UG >= 1 && UG <= 256 && slp >= 1 && slp <= UG && ns >= nlev && cbn >= 1 && W >= 1 && W <= 256);
  const long long ue0 = (g.g0 + gi) * UG;
  const long long tile0 = ue0 / slp;   // (W > 1: slp = 1)
  const int ntg = UG / slp;
  const int nslice = (int)((ba.j.chunk + 63) / 64);
  const long long rem_e = j.chunk - j.main_e;
  R2* const lf = reinterpret_cast<R2*>(cc_lds) + CC_ARGS_E;   // [column][unit][ns]: the condition tracer, then a value tracer
  R2* const lw = lf + (long long)ga.CB * UG * ns;      // [unit][ns]: rho * adz
  R2* const llo = lw + (long long)UG * ns;            // [unit][ns]: lo of the slot's instance and tall level
  R2* const lhi = llo + (long long)UG * ns;           // [unit][ns]: hi
  int* const wt = reinterpret_cast<int*>(lhi + (long long)UG * ns);   // windowed: (k0, lo, hi, -) of the W windows
  const R2* const f0 = static_cast<const R2*>(j.prv);
  constexpr bool has_lo = HL, has_hi = HH;
  const int ntr_v = ba.ntr;   // the value tracers (0 without cpath: the launcher sees to it)
  // the lane's pair
  const int ci = tid / UG, ug = tid - ci * UG;
  const bool act = ci < cbn;
  const long long ue = ue0 + ug;

  if (WIN) {   // the window table, once: the owned levels of window h as levels of its chunk slot
    // (the launcher admits W <= 256, hence nz < 2^15: told to the compiler, the divides of the geometry are 32-bit ones)
    const int nzt = ba.sel.nz;
    __builtin_assume(nzt >= 2 && nzt < 32768);
    for (int h = tid; h < W; h += 256) {
      __builtin_assume(h >= 0 && h < 256);
      int k0 = 0, nz_w, own0 = 1, own1 = 0;
      if (mpd_level_window(nzt, h, &k0, &nz_w, &own0, &own1) != W) { k0 = 0; own1 = own0 - 1; }
      wt[4 * h] = k0; wt[4 * h + 1] = own0 - 1 - k0; wt[4 * h + 2] = max(own1 - k0, own0 - 1 - k0); wt[4 * h + 3] = 0;
    }
    __syncthreads();
  }
  // A zero the compiler cannot see through and must keep per lane (the unused fourth word of a window's table entry, read
  // at a lane's own address): added to the LDS column stride and the column step of f, it keeps their multiples -- eight
  // each in the staging loops, hoisted out of the whole nest -- in vector registers, where there is room, and out of the
  // scalar ones, where a windowed plan's nest had none left.
  const int vz = WIN ? wt[4 * min(lane, W - 1) + 3] : 0;
  const int csv = UG * ns + vz;   // LDS elements from a column to the next

  // a tracer's columns of the batch, window m of the group's tiles: a wave per tile, lane -> element of the chunk
  auto stage = [&](const R2* const f, const int m) __attribute__((always_inline)) {
    for (int tg = wave; tg < ntg; tg += 4) {
      const long long tile = (tile0 + tg) * W + m;
      if (tile < g.t0 || tile > g.t1) continue;
      int lo = 0, hi = (int)j.chunk;
      if (WIN) {   // the owned levels of the halves that belong to the block
        lo = nlev; hi = 0;
#pragma unroll
        for (int h = 0; h < E::N; ++h) {
          long long sl;
          int k0, l0, l1;
          slot_levels<WIN>(b.sel, wt, nlev, tile0 + tg, E::N, m * E::N + h, &sl, &k0, &l0, &l1);   // (slp = 1: a unit per W tiles)
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
        const long long cstep = (in_main ? j.main_e : rem_e) + vz;
        const R2* const p = src + (in_main ? e : (long long)j.ncol_p * j.main_e + (e - j.main_e)) + (3 + c0) * cstep;   // column 1 = slot 3
        R2* const d = lf + (long long)(tg * slp + es) * ns + ek;
        for (int i = 0; i < cbn; i += NB) {
          R2 v[NB];
#pragma unroll
          for (int u = 0; u < NB; ++u) v[u] = p[(long long)min(i + u, cbn - 1) * cstep];
#pragma unroll
          for (int u = 0; u < NB; ++u)
            if (in && i + u < cbn) d[(i + u) * csv] = v[u];
        }
      }
    }
  };

  // W = 1: a value tracer's sum is whole after its walk and is stored at once -- one pass, the condition staged once for
  // all of them.  Windowed: the sums of up to CC_TCH tracers run across the windows in registers; more tracers, more passes.
  constexpr int MW = WIN ? CC_MW_WIN : CC_MW;
  constexpr int TCH = WIN ? CC_TCH : 1;
  int kc[E::N], kb[E::N], kt[E::N];   // counts and tall levels as integers: exact, and the reals of the definition below 2^24
  const int npass = WIN ? max(1, (ntr_v + TCH - 1) / TCH) : 1;
  bool fresh = true;   // nothing has read LDS yet
  for (int pass = 0; pass < npass; ++pass) {
    const int nt = WIN ? min(TCH, ntr_v - pass * TCH) : ntr_v;
    R acc[E::N][TCH];   // windowed: [instance of the unit][tracer of the pass], the tracer in turn at position 0
#pragma unroll
    for (int a = 0; a < E::N; ++a)
#pragma unroll
      for (int u = 0; u < TCH; ++u) acc[a][u] = 0;
#pragma unroll
    for (int a = 0; a < E::N; ++a) kc[a] = kb[a] = kt[a] = 0;   // (every pass forms them again; the last one's are stored)

    for (int m = 0; m < W; ++m) {
      if (!fresh) __syncthreads();   // the walks before are through with LDS
      fresh = false;
      stage(f0 + (long long)b.tc * j.prv_tstride, m);
      // the rows of the group's slots.  The weight, one rounded multiply per level: lanes along the levels, as rho and adz lie
      for (int x = tid; x < UG * nlev; x += 256) {
        const int u2 = x / nlev, kk = x - u2 * nlev;
        const long long ue2 = ue0 + u2;
        const long long tile = ue2 / slp * W + m;
        if (tile < g.t0 || tile > g.t1) continue;
        const long long o = tile * b.kc_tile_stride + (long long)(ue2 % slp) * nlev + kk;
        const R2 r2 = static_cast<const R2*>(b.rho)[o], a2 = static_cast<const R2*>(b.adz)[o];
        R2 w2;
#pragma unroll
        for (int h = 0; h < E::N; ++h) E::at(w2, h) = E::get(r2, h) * E::get(a2, h);
        lw[u2 * ns + kk] = w2;
      }
      // the bounds of the tall level a slot's level stands for: lanes along the INSTANCES, as lo and hi lie (reference layout,
      // instance fastest: a group's reals of a level are one or two whole lines)
      const int ur = UG * E::N;   // reals of the group (a power of two)
      for (int x = tid; x < ur * nlev; x += 256) {
        const int kk = x / ur, r = x - kk * ur, u2 = r / E::N, h = r - u2 * E::N;
        const long long ue2 = ue0 + u2;
        const long long tile = ue2 / slp * W + m;
        if (tile < g.t0 || tile > g.t1) continue;
        long long sl;
        int k0, l0, l1;
        slot_levels<WIN>(b.sel, wt, nlev, ue2, E::N, m * E::N + h, &sl, &k0, &l0, &l1);
        R lv = 0, hv = 0;
        if (kk >= l0 && kk < l1) {
          const long long ob = (sl - b.sel.sl0) + b.sel.n * (long long)(k0 + kk);
          if (has_lo) lv = static_cast<const R*>(b.lo)[ob];
          if (has_hi) hv = static_cast<const R*>(b.hi)[ob];
        }
        reinterpret_cast<R*>(llo)[(u2 * ns + kk) * E::N + h] = lv;
        reinterpret_cast<R*>(lhi)[(u2 * ns + kk) * E::N + h] = hv;
      }
      __syncthreads();

      // ---- the condition: a lane per (unit, column), its levels in rising order; the in-bit of window level kk is bit
      // kk & 31 of word kk >> 5 (the words pass through position 0 of the lane's register array: rotate_in)
      const long long tile = ue / slp * W + m;
      const bool tile_in = tile >= g.t0 && tile <= g.t1;
      const R2* const pf = lf + ci * csv + ug * ns;
      const R2* const pw = lw + ug * ns;
      const R2* const pl = llo + ug * ns;
      const R2* const ph = lhi + ug * ns;
      unsigned mk[E::N][MW];
      int lv0[E::N], lv1[E::N];
      long long isl[E::N];
#pragma unroll
      for (int h = 0; h < E::N; ++h) {
        long long sl;
        int k0, lo, hi;
        slot_levels<WIN>(b.sel, wt, nlev, ue, E::N, m * E::N + h, &sl, &k0, &lo, &hi);
        if (!tile_in || !act) hi = lo;
        lv0[h] = lo; lv1[h] = hi; isl[h] = sl;
        const bool fst = sl == ue * E::N;   // which of the unit's instances the slot belongs to
        int cn = fst ? kc[0] : kc[E::N - 1], bo = fst ? kb[0] : kb[E::N - 1], to = fst ? kt[0] : kt[E::N - 1];
#pragma unroll
        for (int w = 0; w < MW; ++w) mk[h][w] = 0u;
#pragma nounroll
        for (int w = 0; w < MW; ++w) {   // (a run-time loop: unrolled, its compare masks overflow the scalar registers)
          unsigned bits = 0u;
          if (w * 32 < hi && w * 32 + 32 > lo) {
            const int kend = min(hi, w * 32 + 32);
#pragma nounroll
            for (int kk = max(w * 32, lo & ~7); kk < kend; kk += NB) {
              R2 c[NB], l[NB], u_[NB];
#pragma unroll
              for (int u = 0; u < NB; ++u) {
                const int kx = min(max(kk + u, lo), hi - 1);
                c[u] = pf[kx];
                l[u] = pl[kx];
                u_[u] = ph[kx];
              }
              unsigned byte = 0u;
#pragma unroll
              for (int u = 0; u < NB; ++u) {
                const R cv = E::get(c[u], h);
                const bool in = (!has_lo || cv > E::get(l[u], h)) && (!has_hi || cv <= E::get(u_[u], h));
                byte |= (in ? 1u : 0u) << u;
              }
              bits |= byte << (kk & 31);   // (kk is a multiple of 8)
            }
            // the levels of the word outside [lo, hi) were read clamped: their bits go
            const int b0 = max(lo - w * 32, 0), b1 = min(hi - w * 32, 32);
            bits &= (b1 >= 32 ? ~0u : (1u << b1) - 1u) & ~((1u << b0) - 1u);
            if (bits) {   // q = q + 1 per level that is in; the first and the last of them
              cn += __popc(bits);
              if (bo == 0) bo = k0 + w * 32 + __ffs((int)bits);
              to = k0 + w * 32 + 32 - __clz((int)bits);
            }
          }
          rotate_in(mk[h], bits);   // (word w comes to rest at mk[h][w] behind the last step)
        }
        if (fst) { kc[0] = cn; kb[0] = bo; kt[0] = to; } else { kc[E::N - 1] = cn; kb[E::N - 1] = bo; kt[E::N - 1] = to; }
      }

      // ---- the value tracers through the same columns of LDS, each summed under the bits
#pragma nounroll
      for (int u3 = 0; u3 < nt; ++u3) {
        __syncthreads();   // the walk before is through with the columns
        stage(f0 + (long long)(b.first + pass * TCH + u3) * j.prv_tstride, m);
        __syncthreads();
#pragma unroll
        for (int h = 0; h < E::N; ++h) {
          const int lo = lv0[h], hi = lv1[h];
          if (hi <= lo) continue;
          const bool fst = isl[h] == ue * E::N;
          R sum = 0;
          if constexpr (WIN) sum = fst ? acc[0][0] : acc[E::N - 1][0];
#pragma nounroll
          for (int w = 0; w < MW; ++w) {
            const unsigned bits = mk[h][0];
            rotate_in(mk[h], bits);     // (word w + 1 to the front; MW steps leave the words where they were)
            if (bits == 0u) continue;   // (bits lie inside [lo, hi) only)
            const int kend = min(hi, w * 32 + 32);
#pragma nounroll
            for (int kk = max(w * 32, lo & ~7); kk < kend; kk += NB) {
              if (((bits >> (kk & 31)) & 0xffu) == 0u) continue;   // (none of the eight is in: nothing to add)
              R2 v[NB], wv[NB];
#pragma unroll
              for (int u = 0; u < NB; ++u) {
                const int kx = min(max(kk + u, lo), hi - 1);
                v[u] = pf[kx];
                wv[u] = pw[kx];
              }
#pragma unroll
              for (int u = 0; u < NB; ++u) {
                const R t = E::get(wv[u], h) * E::get(v[u], h);
                sum = (bits >> ((kk + u) & 31)) & 1u ? sum + t : sum;
              }
            }
          }
          if constexpr (WIN) { if (fst) acc[0][0] = sum; else acc[E::N - 1][0] = sum; }
          else static_cast<R*>(b.cpath)[(isl[h] - b.sel.sl0) + b.sel.n * ((c0 + ci) + (long long)nx * u3)] = sum;   // (hi > lo: an instance of the block)
        }
        if constexpr (WIN) {   // the next tracer's sums to the front
#pragma unroll
          for (int a = 0; a < E::N; ++a) rotate_in(acc[a], acc[a][0]);
        }
      }
      if constexpr (WIN) {   // ... and the first tracer's again: TCH steps in all
#pragma nounroll
        for (int u3 = nt; u3 < TCH; ++u3) {
#pragma unroll
          for (int a = 0; a < E::N; ++a) rotate_in(acc[a], acc[a][0]);
        }
      }
    }

    // (the lane's own test and width once more behind the nest, through vz: formed here, not carried across it in scalars)
    if (WIN && ci + vz * (pass + 1) < cbn) {   // (nt = 0 without cpath: nothing is stored; vz times the pass: not hoisted)
#pragma unroll
      for (int a = 0; a < E::N; ++a) {
        const long long sl = ue * E::N + a;
        if (sl < b.sel.sl0 || sl >= b.sel.sl0 + b.sel.n) continue;   // the phantom, the partner of a split pair, a neighbour in the group
#pragma nounroll
        for (int u3 = 0; u3 < nt; ++u3) {
          static_cast<R*>(b.cpath)[(sl - b.sel.sl0) + b.sel.n * ((c0 + ci) + (long long)(nx + vz) * (pass * TCH + u3))] = acc[a][0];
          rotate_in(acc[a], acc[a][0]);
        }
      }
    }
  }
  if (ci + vz >= cbn) return;
#pragma unroll
  for (int a = 0; a < E::N; ++a) {
    const long long sl = ue * E::N + a;
    if (sl < b.sel.sl0 || sl >= b.sel.sl0 + b.sel.n) continue;   // padding, phantom, the partner of a split pair, a neighbour in the group
    const long long o = (sl - b.sel.sl0) + b.sel.n * (long long)(c0 + ci);
    if (b.kcnt) static_cast<R*>(b.kcnt)[o] = (R)kc[a];
    if (b.kbot) static_cast<R*>(b.kbot)[o] = (R)kb[a];
    if (b.ktop) static_cast<R*>(b.ktop)[o] = (R)kt[a];
  }
}

// Reference layout: element (sl, column i, level k, tracer t) at f + sl + ld * ((i + 2) + (nx + 6) * ((k - 1) + nlev * t)), rho,
// adz at sl + ld * (k - 1), lo and hi at b + n * (k - 1).  x: instances of the block, y: columns.
template <typename R>
__global__ void __launch_bounds__(256) ref_column_cond_kernel(const R* f, const R* rho, const R* adz, const long long ld, const long long sl0,
                                                             const long long n, const int nx, const int nlev, const int tc, const R* lo,
                                                             const R* hi, R* kcnt, R* kbot, R* ktop, R* cpath, const int first, const int ntr) {
  const long long bi = (long long)blockIdx.x * 256 + threadIdx.x;
  if (bi >= n) return;
  const long long sl = sl0 + bi, step = ld * (nx + 6), tstep = step * nlev;
  for (long long i = blockIdx.y; i < nx; i += gridDim.y) {
    const R* const pc = f + sl + ld * (i + 3) + tstep * tc;
    if (kcnt || kbot || ktop) {
      R cn = 0, bo = 0, to = 0;
      for (int k = 0; k < nlev; k += NB) {
        R c[NB], l[NB], h[NB];
#pragma unroll
        for (int u = 0; u < NB; ++u) {
          const long long kx = min(k + u, nlev - 1);
          c[u] = pc[kx * step];
          l[u] = lo ? lo[bi + n * kx] : (R)0;
          h[u] = hi ? hi[bi + n * kx] : (R)0;
        }
#pragma unroll
        for (int u = 0; u < NB; ++u) {
          const bool in = k + u < nlev && (!lo || c[u] > l[u]) && (!hi || c[u] <= h[u]);
          const R lev = (R)(k + u + 1);
          cn = in ? cn + (R)1 : cn;
          bo = in && bo == (R)0 ? lev : bo;
          to = in ? lev : to;
        }
      }
      if (kcnt) kcnt[bi + n * i] = cn;
      if (kbot) kbot[bi + n * i] = bo;
      if (ktop) ktop[bi + n * i] = to;
    }
    if (!cpath) continue;
    for (int jt = 0; jt < ntr; ++jt) {
      const R* const pv = pc + tstep * (long long)(first + jt - tc);   // (a signed offset)
      R sum = 0;
      for (int k = 0; k < nlev; k += NB) {
        R c[NB], v[NB], l[NB], h[NB], rv[NB], av[NB];
#pragma unroll
        for (int u = 0; u < NB; ++u) {
          const long long kx = min(k + u, nlev - 1);
          c[u] = pc[kx * step];
          v[u] = pv[kx * step];
          l[u] = lo ? lo[bi + n * kx] : (R)0;
          h[u] = hi ? hi[bi + n * kx] : (R)0;
          rv[u] = rho[sl + ld * kx];
          av[u] = adz[sl + ld * kx];
        }
#pragma unroll
        for (int u = 0; u < NB; ++u) {
          const bool in = k + u < nlev && (!lo || c[u] > l[u]) && (!hi || c[u] <= h[u]);
          const R w = rv[u] * av[u];
          const R t = w * v[u];
          sum = in ? sum + t : sum;
        }
      }
      cpath[bi + n * (i + (long long)nx * jt)] = sum;
    }
  }
}

// cover(b) = the columns with kcnt(b, i) > 0; mass(b, j) = the sequential sum over i of cpath(b, i, j).  x: instances of
// the block, y: tracers (row ntr: cover).
template <typename R>
__global__ void __launch_bounds__(256) column_cond_tail_kernel(const R* kcnt, const R* cpath, const long long n, const int nx, const int ntr,
                                                              R* cover, R* mass) {
  const long long bi = (long long)blockIdx.x * 256 + threadIdx.x;
  if (bi >= n) return;
  const long long rows = (mass ? ntr : 0) + (cover ? 1 : 0);
  for (long long r = blockIdx.y; r < rows; r += gridDim.y) {
    const bool cov = !mass || r == ntr;
    const R* const p = cov ? kcnt + bi : cpath + bi + n * nx * r;
    R sum = 0;
    for (int i = 0; i < nx; i += NB) {
      R v[NB];
#pragma unroll
      for (int u = 0; u < NB; ++u) v[u] = p[n * min(i + u, nx - 1)];
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        if (i + u >= nx) continue;
        if (cov) sum = v[u] > (R)0 ? sum + (R)1 : sum;
        else sum = sum + v[u];
      }
    }
    if (cov) cover[bi] = sum; else mass[bi + n * r] = sum;
  }
}

hipError_t column_cond_tail(const void* kcnt, const void* cpath, int elem_bytes, long long n, int nx, int ntr, void* cover, void* mass,
                            hipStream_t stream) {
  if (!cover && !mass) return hipSuccess;
  if ((cover && !kcnt) || (mass && !cpath)) return hipErrorInvalidValue;
  dim3 grid, block(256);
  if (ref_block_grid(n, (mass ? ntr : 0) + (cover ? 1 : 0), &grid) != hipSuccess) return hipErrorInvalidValue;
  return ref_real(elem_bytes, [&](auto r) {
    typedef decltype(r) R;
    hipLaunchKernelGGL((column_cond_tail_kernel<R>), grid, block, 0, stream, static_cast<const R*>(kcnt), static_cast<const R*>(cpath), n, nx,
                       ntr, static_cast<R*>(cover), static_cast<R*>(mass));
    return hipGetLastError();
  });
}

// the instantiation of a call: fp32 pairs or fp64, windowed or not, which bounds are given (one of them is)
typedef void (*WmKernel)(const MpdataColumnCondJob, const CcGeom);
template <typename R2, bool WIN>
WmKernel wm_kernel_bounds(const bool lo, const bool hi) {
  return lo && hi ? wm_column_cond_kernel<R2, WIN, true, true>
         : lo     ? wm_column_cond_kernel<R2, WIN, true, false>
                  : wm_column_cond_kernel<R2, WIN, false, true>;
}
WmKernel wm_kernel(const bool f32, const bool win, const bool lo, const bool hi) {
  return f32 ? (win ? wm_kernel_bounds<float2, true>(lo, hi) : wm_kernel_bounds<float2, false>(lo, hi))
             : (win ? wm_kernel_bounds<double, true>(lo, hi) : wm_kernel_bounds<double, false>(lo, hi));
}

bool cond_args_ok(int ntr_all, int tc, const void* lo, const void* hi, const void* kcnt, const void* kbot, const void* ktop,
                  const void* cpath, const void* cover, const void* mass, int first, int ntr) {
  if (tc < 0 || tc >= ntr_all || (!lo && !hi)) return false;
  if (!kcnt && !kbot && !ktop && !cpath && !cover && !mass) return false;
  if ((cover && !kcnt) || (mass && !cpath)) return false;
  return !cpath || (first >= 0 && ntr >= 1 && first <= ntr_all - ntr);
}

}  // namespace

hipError_t mpdata_column_cond_wm(const MpdataColumnCondJob& b, hipStream_t stream) {
  WmGrid wg;
  const MpdataLayoutJob& j = b.j;
  if (!b.rho || !b.adz || j.prv_col0 != 0 || j.ncols != j.ncol_p || b.kc_tile_stride < j.chunk || j.nlev > 32 * (b.sel.W > 1 ? CC_MW_WIN : CC_MW) ||
      !cond_args_ok(j.ntr, b.tc, b.lo, b.hi, b.kcnt, b.kbot, b.ktop, b.cpath, b.cover, b.mass, b.first, b.ntr))
    return hipErrorInvalidValue;
  hipError_t e = wm_block_grid(j, b.sel, 1, &wg);
  if (e != hipSuccess) return e;
  // three rows next to the columns: rho * adz, lo, hi; 16 units = one 128-byte line of an (n, nx) row per column; the
  // kernel counts units in long long
  ColGroups cg;
  const bool win = b.sel.W > 1;
  if (b.sel.W > 256 || (win && b.sel.nz >= 32768) || !col_groups_batched(j, b.sel, wg, CC_LDS_ELEMS, /*fixed: the arguments and the window table*/ CC_ARGS_E + (win ? 2 * b.sel.W : 0), /*rows*/ 3,
                                            /*unit_mul*/ 0, &cg))
    return hipErrorInvalidValue;
  CcGeom g;
  g.t0 = wg.t0; g.t1 = wg.t0 + wg.ntile - 1;
  col_groups_fill(cg, &g);
  g.ncb = cg.ncb;
  const unsigned blocks = (unsigned)(g.ngroup * g.ncb);
  MpdataColumnCondJob bk = b;
  if (!bk.cpath) bk.first = bk.ntr = 0;   // (the kernel takes the number of value tracers from ntr alone)
  hipLaunchKernelGGL(wm_kernel(b.sel.ipe == 2, win, b.lo != nullptr, b.hi != nullptr), dim3(blocks), dim3(256), (size_t)cg.lds_e * 8, stream,
                     bk, g);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  return column_cond_tail(b.kcnt, b.cpath, 8 / b.sel.ipe, b.sel.n, j.ncol_p - 6, b.ntr, b.cover, b.mass, stream);
}

hipError_t mpdata_column_cond_ref(const void* f, const void* rho, const void* adz, int elem_bytes, long long ld, long long sl0,
                                  long long n, int nx, int nlev, int ntr_all, int tc, const void* lo, const void* hi, void* kcnt,
                                  void* kbot, void* ktop, void* cpath, void* cover, void* mass, int first, int ntr, hipStream_t stream) {
  if (!f || !rho || !adz || ld < 1 || sl0 < 0 || n < 1 || sl0 + n > ld || nx < 1 || nlev < 1 || (elem_bytes != 4 && elem_bytes != 8) ||
      !cond_args_ok(ntr_all, tc, lo, hi, kcnt, kbot, ktop, cpath, cover, mass, first, ntr))
    return hipErrorInvalidValue;
  dim3 grid, block(256);
  if (ref_block_grid(n, nx, &grid) != hipSuccess) return hipErrorInvalidValue;
  const hipError_t e = ref_real(elem_bytes, [&](auto r) {
    typedef decltype(r) R;
    hipLaunchKernelGGL((ref_column_cond_kernel<R>), grid, block, 0, stream, static_cast<const R*>(f), static_cast<const R*>(rho),
                       static_cast<const R*>(adz), ld, sl0, n, nx, nlev, tc, static_cast<const R*>(lo), static_cast<const R*>(hi),
                       static_cast<R*>(kcnt), static_cast<R*>(kbot), static_cast<R*>(ktop), static_cast<R*>(cpath), first, ntr);
    return hipGetLastError();
  });
  if (e != hipSuccess) return e;
  return column_cond_tail(kcnt, cpath, elem_bytes, n, nx, ntr, cover, mass, stream);
}
