// mpdata_cell_add.hip -- per-cell sources of f, in place (include/mpdata_hip.h 3p, mpdata_cell_add.h): f += c * s with a
// field s that differs in every cell and tracer -- radiative heating, the tendency of a physics scheme the library does
// not own, a source confined to some columns -- optionally clipped at zero, with the applied increment summed over the
// interior columns.  The second call that reads a per-cell field in the reference layout where it lies
// (mpdata_sediment.hip is the first) and the first without a vertical neighbour.  A kernel of its own outside the run:
// nothing is fused into the plan kernels, nothing is kept between calls.
//   plan layout: the groups, rounds and the walk of f of mpdata_sediment.hip -- a workgroup owns the whole tiles of a
//     GROUP of UG adjacent 8-byte elements of the instance axis (units), a wave per 64-element slice of a tile's column
//     chunk, lane -> element e = s * nlev + kk, the interior column slots 3 .. nx+2 as linear streams with the main / rest
//     split, a wave visits the tiles of its group in ROUNDS of 4 / nslice tiles.  Per batch of CB columns:
//       the four waves copy the group's rows of s into ONE OF TWO LDS buffers (batch parity) as [column][unit][level]
//       with an odd level stride -- on plain plans that stage whole elements from registers, which the threads then load
//       with their share of the NEXT batch, so that those loads fly while this batch computes --; the loads of f of the
//       first round are issued; (S) barrier; per round the LDS reads, the arithmetic and the stores.
//     A lane reads and writes its own element of f and no other, and no two lanes share one: f needs no ordering.  (S) is
//     the only barrier of a batch; why one is enough with two buffers: DESIGN.md 4.19.
//     A windowed plan: a workgroup per group AND window (blockIdx.y), staged by tall level from the caller's s.
//     The running sums of dsum live in LDS, one slot per (round, thread), touched by that thread alone; without dsum the
//     kernel is another instantiation that has neither the sums nor their LDS.
//   reference layout: one thread per instance and (level, tracer) row, coalesced along sl, marching i; in place.
// Built with -ffp-contract=off: every operation of the definition is rounded once, in its association.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>

#include "mpdata_cell_add.h"

namespace {

using namespace wm_walk;

// (LDS_ELEMS, the LDS of a workgroup at most, and the column groups of the launch: mpdata_wm_walk.h)

__device__ inline double pos(double a) { return fmax(a, 0.0); }
__device__ inline float pos(float a) { return fmaxf(a, 0.0f); }

// Per-lane conditions that live across a round are kept as bit masks in vector registers and applied to the bit patterns,
// as in mpdata_sediment.hip: held as lane masks they would take two scalar registers each.  The selections are exact.
__device__ inline int vmask(const bool c) {
  int m = c ? -1 : 0;
  asm volatile("" : "+v"(m));
  return m;
}
__device__ inline float pick(const float a, const float b, const int m) {   // m ? a : b
  return __int_as_float((__float_as_int(a) & m) | (__float_as_int(b) & ~m));
}
__device__ inline double pick(const double a, const double b, const int m) {
  const long long mm = ((long long)m << 32) | (unsigned)m;
  return __longlong_as_double((__double_as_longlong(a) & mm) | (__double_as_longlong(b) & ~mm));
}

// The workgroups of the plan-layout kernel: units, groups and batches as in mpdata_sediment.hip (SedArgs).
struct CellArgs {
  void* f;                    // the plan side of f, first tracer of the call
  const void* s;
  void* dsum;
  double c;
  long long n, sl0, nslots;   // the block; the plan's slots (ncrms * W)
  long long tstride, tile_stride;
  int chunk, main_e, ncol_p, nlev, slp;
  int W, nz;
  int t0, t1;                 // tiles the block touches
  int g0, ngroup;             // first group, groups
  int UG, CB, ns;             // ns: level stride in LDS (odd)
  int ush;                    // UG = 1 << ush
  int nslice, nround;
  int clip;
};

// Plan layout.  blockIdx.x = tracer * ngroup + group; R2: one 8-byte element (double, or the float2 of two adjacent
// slots); WIN: a windowed plan (W > 1, one slot per tile), a workgroup per window (blockIdx.y); PAIRS: s is staged in
// whole 8-byte elements (fp64; an fp32 block whose pairs are whole and 8-byte aligned in s), else in single reals; DSUM:
// the sums are kept and written.
template <typename R2, bool WIN, bool PAIRS, bool DSUM>
__global__ void __launch_bounds__(256) wm_cell_add_kernel(const CellArgs g) {
  typedef Elem<R2> E;
  typedef typename E::R R;
  constexpr int N = E::N;
  extern __shared__ __align__(8) unsigned char cad_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int gi = blockIdx.x % g.ngroup;
  const int tr = blockIdx.x / g.ngroup;
  const int nlev = g.nlev, nx = g.ncol_p - 6, slp = WIN ? 1 : g.slp, W = WIN ? g.W : 1, ns = g.ns, UG = g.UG;
  const int nslice = g.nslice, tpw = 4 / nslice, ntg = UG / slp;
  const int nzm = g.nz - 1;
  const long long n = g.n, sl0 = g.sl0;
  const int ue0 = (g.g0 + gi) * UG;
  const int lbuf = g.CB * UG * ns;                      // elements of one staging buffer
  R2* const lw0 = reinterpret_cast<R2*>(cad_lds);       // 2 x [column][unit][ns]: s
  R2* const lacc = lw0 + 2 * lbuf;                      // DSUM: [round][thread]: the running sums
  int* const lwin = reinterpret_cast<int*>(lacc + (DSUM ? g.nround * 256 : 0));   // WIN: [half]{k0, own0, own1, -}
  R2* const f = static_cast<R2*>(g.f) + (long long)tr * g.tstride;
  const R* const sp = static_cast<const R*>(g.s) + n * ((long long)nx * nzm * tr);
  const R cf = (R)g.c;   // the one rounding of the factor
  const int clipm = vmask(g.clip != 0);   // (a mask as the per-lane ones below: no scalar register held across the loops)

  // the lane's element of a chunk (the same in every tile the wave visits)
  const bool wave_in = wave < tpw * nslice;   // (three slices: the fourth wave idles)
  const int slice = wave % nslice;
  const int e0 = slice * 64 + lane;
  const bool lane_in = wave_in && e0 < g.chunk;
  const int e = lane_in ? e0 : 0;   // (idle lanes read element 0 and store nothing)
  const int s = e / nlev, kk = e - s * nlev;
  const bool main_o = e < g.main_e;
  const int so = main_o ? g.main_e : g.chunk - g.main_e;   // column stride
  const int oo = main_o ? e : g.ncol_p * g.main_e + (e - g.main_e);

  // a windowed plan: blockIdx.y is the tile m of every unit of the group; the constants of its (two) windows go through LDS
  const int m = WIN ? blockIdx.y : 0;
  if (WIN) {
    if (tid < N) {
      int k0 = 0, nz_w, own0 = 1, own1 = 0;
      if (mpd_level_window(g.nz, (m * N + tid) % W, &k0, &nz_w, &own0, &own1) != W) own1 = own0 - 1;
      lwin[4 * tid] = k0; lwin[4 * tid + 1] = own0; lwin[4 * tid + 2] = own1;
    }
    __syncthreads();   // (W) the window constants are in LDS
  }
  // the window each half of tile (unit, m) is: slot q = (unit * W + m) * N + h is window q % W of instance q / W
  int k0h[N], own0h[N], own1h[N], dih[N];
#pragma unroll
  for (int h = 0; h < N; ++h) {
    k0h[h] = 0; own0h[h] = 1; own1h[h] = nzm;
    dih[h] = h;
    if (WIN) {
      dih[h] = (m * N + h) / W;
      asm volatile("" : "+v"(dih[h]));   // (wave-uniform, but the fp32 windowed kernel has no scalar register to spare for it)
      k0h[h] = lwin[4 * h]; own0h[h] = lwin[4 * h + 1]; own1h[h] = lwin[4 * h + 2];
    }
  }
  // ---- the staging of s, a thread's share of it kept in registers between its loads and its LDS stores: a row of the
  // group is UG units, adjacent in s wherever the slots are adjacent instances (a row is a power of two of staged items,
  // 256 at most: a thread keeps its place in the row and walks the rows of a batch in steps of 256 / row length).  A
  // buffer holds LDS_ELEMS / 2 elements at most, so a thread has MAXJ items of a batch at most.
  typedef typename std::conditional<PAIRS, R2, R>::type T;   // the staged item: a whole 8-byte element, or a single real
  constexpr int TN = PAIRS ? 1 : N;                          // items per element
  // PRE: a thread's items of the NEXT batch are loaded into registers while this batch computes.  Single reals and
  // windowed plans are staged by the plain loop below: 20 reals in registers would halve the waves a SIMD holds, and the
  // windowed kernels have no scalar registers left for the walk (the build's report shows spills; the test refuses them).
  constexpr bool PRE = PAIRS && !WIN;
  constexpr int MAXJ = PRE ? LDS_ELEMS / 2 / 256 : 1;
  const int lsh = g.ush + (TN - 1);
  const int lidx = tid & ((1 << lsh) - 1), u2 = lidx / TN, sh = lidx - u2 * TN;
  const long long ssl = (long long)(ue0 + u2) * N + (PAIRS ? 0 : (sh ? dih[N - 1] : dih[0]));
  const bool sin = ssl >= sl0 && ssl + (PAIRS ? N : 1) <= sl0 + n;
  const T* const ssrc = reinterpret_cast<const T*>(sp + (sin ? ssl - sl0 : 0));
  const long long snT = PAIRS ? n / N : n;                   // items between two columns of s
  const int sk0 = sh ? k0h[N - 1] : k0h[0];
  // the walk over a thread's rows, row0 + j * rstep: the column ci and the level k2 of a row advance by the quotient and
  // the remainder of rstep / nlev, with one carry at most; the addresses advance with them (no divide in the loops)
  const int rsh = 8 - lsh, rstep = 1 << rsh, row0 = tid >> lsh;
  const int ci0 = row0 / nlev, k20 = row0 - ci0 * nlev, dq = rstep / nlev, dr = rstep - dq * nlev;
  const long long gstep = snT * (dq + (long long)nx * dr), gcarry = snT * (1 - (long long)nx * nlev);
  const T* const ssrc0 = ssrc + snT * (ci0 + (long long)nx * (sk0 + k20));
  const int l0 = ((ci0 * UG + u2) * ns + k20) * TN + sh;
  const int lstep = (dq * UG * ns + dr) * TN, lcarry = (UG * ns - nlev) * TN;
  T sreg[MAXJ];
  // the loads of the batch at column c0b (cbnb columns): all of a thread's items in flight at once
  auto stage_load = [&](const int c0b, const int cbnb) {
    const int nj = row0 < cbnb * nlev ? (cbnb * nlev - row0 + rstep - 1) >> rsh : 0;
    const T* ptr = ssrc0 + snT * c0b;
    int k2 = k20;
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
      // (not predicated: a row past the batch reads the first item of
      // the unit's s instead -- an address inside s; what it brings reaches no result.  A unit outside the block reads
      // the block's first unit: its lanes select nothing of it.)
      sreg[j] = *(j < nj ? ptr : ssrc);
      ptr += gstep; k2 += dr;
      if (k2 >= nlev) { k2 -= nlev; ptr += gcarry; }
    }
  };
  // ... and their stores into the buffer lw as [column][unit][ns]
  auto stage_store = [&](R2* const lw, const int cbnb) {
    T* const l = reinterpret_cast<T*>(lw);
    const int nj = row0 < cbnb * nlev ? (cbnb * nlev - row0 + rstep - 1) >> rsh : 0;
    int li = l0, k2 = k20;
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
      if (j < nj) l[li] = sreg[j];
      li += lstep; k2 += dr;
      if (k2 >= nlev) { k2 -= nlev; li += lcarry; }
    }
  };
  if constexpr (PRE) stage_load(0, min(g.CB, nx));
  int par = 0;
  for (int c0 = 0; c0 < nx; c0 += g.CB, par ^= 1) {
    const int cbn = min(g.CB, nx - c0);
    R2* const lw = lw0 + par * lbuf;   // the buffer of this batch: the one the batch before did not read
    if constexpr (PRE) {
      stage_store(lw, cbn);
      // the next batch's s is on its way while this batch computes
      if (c0 + g.CB < nx) stage_load(c0 + g.CB, min(g.CB, nx - c0 - g.CB));
    } else {
      for (int row = row0; row < cbn * nlev; row += rstep) {
        const int ci = row / nlev, k2 = row - ci * nlev;
        T v = T();
        if (sin && sk0 + k2 < nzm) v = ssrc[snT * ((c0 + ci) + (long long)nx * (sk0 + k2))];
        reinterpret_cast<T*>(lw)[((ci * UG + u2) * ns + k2) * TN + sh] = v;
      }
    }
    for (int r = 0; r < g.nround; ++r) {
      const int tg = r * tpw + wave / nslice;
      const int tile_r = (ue0 / slp + tg) * W + m;
      const bool task = wave_in && tg < ntg && tile_r >= g.t0 && tile_r <= g.t1;
      const int tile = task ? tile_r : g.t0;   // (an idle wave reads tile t0 and stores nothing)
      const int ug = tg < ntg ? tg * slp + s : 0;
      // per half: the instance and the tall level the slot stands for
      int onm[N], phm[N];
      long long bi[N];
      int kt[N];
      bool any = false;
#pragma unroll
      for (int h = 0; h < N; ++h) {
        const long long q = ((long long)tile * slp + s) * N + h;
        // the phantom half follows the plan's last slot; a windowed plan's is no instance of the block here (sl = ncrms),
        // keeps its bits, and is restored by the caller behind the kernel, as after a seam refresh
        const bool ph = !WIN && N == 2 && (g.nslots & 1) && q == g.nslots;
        const int hq = ph ? 0 : h;   // (unrolled: a constant index or a select)
        const long long sl = WIN ? (long long)(ue0 + tg) * N + dih[hq] : (ph ? q - 1 : q);   // = (ph ? q - 1 : q) / W
        kt[h] = k0h[hq] + kk;
        bool ok = task && lane_in && sl >= sl0 && sl < sl0 + n && kt[h] < nzm;
        if (WIN) ok = ok && kt[h] + 1 >= own0h[hq] && kt[h] + 1 <= own1h[hq];
        onm[h] = vmask(ok);   // else: padding, the partner of a split pair, a neighbour in the group, a level the window does not own
        phm[h] = vmask(ph);
        any = any || ok;
        bi[h] = ok ? sl - sl0 : 0;
      }
      const bool wave_any = __ballot(any) != 0;
      R2* const pf = f + tile * g.tile_stride + oo + (3 + c0) * so;   // column c0 + 1 = slot c0 + 3
      // ---- every load of f of the round (cut by the wave-uniform batch length: every address is a column of the batch)
      R2 v[NB];
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        v[u] = R2();
        if (u < cbn) v[u] = pf[u * so];
      }
      if (r == 0) __syncthreads();   // (S) the batch's s is in LDS; every wave is through with the OTHER buffer
      if (wave_any) {
        R2 acc;
#pragma unroll
        for (int h = 0; h < N; ++h) E::at(acc, h) = 0;
        if (DSUM && c0 > 0) acc = lacc[r * 256 + tid];
        const int anym = onm[0] | onm[N - 1];
        const R2* pw = lw + ug * ns + kk;   // the lane's element of s, a column per step
#pragma unroll
        for (int u = 0; u < NB; ++u) {
          if (u < cbn) {
            const R2 fcur = v[u];
            const R2 s2 = pw[0];
            R2 out = fcur;
#pragma unroll
            for (int h = 0; h < N; ++h) {
              const R f_c = E::get(fcur, h);
              const R p = cf * E::get(s2, h);
              R gv = f_c + p;
              gv = pick(pos(gv), gv, clipm);
              if (DSUM) {
                const R d = gv - f_c;
                E::at(acc, h) = E::get(acc, h) + d;
              }
              E::at(out, h) = pick(gv, f_c, onm[h]);
            }
            if (N == 2) E::at(out, N - 1) = pick(E::get(out, 0), E::get(out, N - 1), phm[N - 1] & onm[N - 1]);
            if (anym) pf[u * so] = out;
            pw += UG * ns;
          }
        }
        if (DSUM) {
          if (c0 + g.CB < nx) {
            lacc[r * 256 + tid] = acc;
          } else {
#pragma unroll
            for (int h = 0; h < N; ++h)
              if (onm[h] && !phm[h]) static_cast<R*>(g.dsum)[bi[h] + n * (kt[h] + (long long)nzm * tr)] = E::get(acc, h);
          }
        }
      }
    }
  }
}

// Reference layout: element (sl, column i, level k, tracer t) at f + sl + ld * ((i + 2) + (nx + 6) * ((k - 1) + nlev * t)),
// s (b, i, k, t) at b + n * ((i - 1) + nx * ((k - 1) + nlev * t)).  x: instances of the block, y: rows r = (k - 1) + nlev * t.
// NB columns of f and s are loaded (indices clamped) before the first store; a thread touches its own row only.
template <typename R>
__global__ void __launch_bounds__(256) ref_cell_add_kernel(R* __restrict__ f, const long long ld, const long long sl0, const long long n,
                                                          const int nx, const long long rows, const R* __restrict__ s, const double c,
                                                          const int clip, R* __restrict__ dsum) {
  const long long bi = (long long)blockIdx.x * 256 + threadIdx.x;
  if (bi >= n) return;
  const R cf = (R)c;
  for (long long r = blockIdx.y; r < rows; r += gridDim.y) {
    R* const p = f + (sl0 + bi) + ld * (3 + (long long)(nx + 6) * r);   // column 1
    const R* const ps = s + bi + n * ((long long)nx * r);
    R acc = 0;
    for (int i = 0; i < nx; i += NB) {
      R v[NB], sv[NB];
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        const int ii = min(i + u, nx - 1);
        v[u] = p[ld * ii];
        sv[u] = ps[n * ii];
      }
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        if (i + u < nx) {
          const R pr = cf * sv[u];
          R gv = v[u] + pr;
          if (clip) gv = pos(gv);
          const R d = gv - v[u];
          acc = acc + d;
          p[ld * (i + u)] = gv;
        }
      }
    }
    if (dsum) dsum[bi + n * r] = acc;
  }
}

template <typename R2, bool DSUM>
void (*wm_kernel(const bool win, const bool pairs))(CellArgs) {
  if constexpr (Elem<R2>::N == 1)   // (an fp64 element is always whole)
    return win ? wm_cell_add_kernel<R2, true, true, DSUM> : wm_cell_add_kernel<R2, false, true, DSUM>;
  else
    return win ? wm_cell_add_kernel<R2, true, false, DSUM> : pairs ? wm_cell_add_kernel<R2, false, true, DSUM> : wm_cell_add_kernel<R2, false, false, DSUM>;
}

}  // namespace

hipError_t mpdata_cell_add_wm(const MpdataCellAddJob& b, hipStream_t stream) {
  WmGrid wg;
  const MpdataLayoutJob& j = b.j;
  if (!b.s || j.prv_col0 != 0 || j.ncols != j.ncol_p) return hipErrorInvalidValue;
  const hipError_t e = wm_block_grid(j, b.sel, j.ntr, &wg);
  if (e != hipSuccess) return e;
  // As in mpdata_sediment_wm: what follows holds for every plan mpdata_plan_create makes, so none of these returns is
  // reached today; a new tiling that breaks one of them must extend the kernel, and fails here, before any launch.
  // Two buffers of s and, with dsum, the running sums; 16 units, fewer where two columns of the group's levels do not
  // fit twice.
  const int slp = j.slp, W = b.sel.W;
  ColGroups cg;
  // (unit, tile and slot-in-LDS arithmetic of the kernel is in int)
  if (!col_groups_tiled(j, b.sel, wg, LDS_ELEMS, /*fixed*/ W > 1 ? 4 : 0, /*rows*/ 0, /*bufs*/ 2, /*sums*/ b.dsum != nullptr,
                        /*wide*/ false, &cg) ||
      (long long)j.ncol_p * j.main_e + j.chunk > 2147483647LL)
    return hipErrorInvalidValue;
  CellArgs g;
  g.f = j.prv; g.s = b.s; g.dsum = b.dsum; g.c = b.c; g.clip = b.clip;
  g.n = b.sel.n; g.sl0 = b.sel.sl0; g.nslots = b.sel.ncrms * W;
  g.tstride = j.prv_tstride; g.tile_stride = j.prv_tile_stride;
  g.chunk = (int)j.chunk; g.main_e = (int)j.main_e; g.ncol_p = j.ncol_p; g.nlev = j.nlev; g.slp = slp;
  g.W = W; g.nz = b.sel.nz;
  g.t0 = (int)wg.t0; g.t1 = (int)(wg.t0 + wg.ntile - 1);
  g.nslice = wg.nslice;
  col_groups_fill(cg, &g);
  g.ush = cg.ush; g.nround = cg.nround;
  // (W > 1: the halves of a pair are windows, not adjacent instances)
  const bool pairs = b.sel.ipe == 2 && W == 1 && b.sel.sl0 % 2 == 0 && b.sel.n % 2 == 0 && reinterpret_cast<uintptr_t>(b.s) % 8 == 0;
  void (*k)(CellArgs) = b.sel.ipe == 1 ? (b.dsum ? wm_kernel<double, true>(W > 1, true) : wm_kernel<double, false>(W > 1, true))
                                       : (b.dsum ? wm_kernel<float2, true>(W > 1, pairs) : wm_kernel<float2, false>(W > 1, pairs));
  hipLaunchKernelGGL(k, dim3((unsigned)(g.ngroup * j.ntr), (unsigned)W), dim3(256), (size_t)cg.lds_e * 8, stream, g);
  return hipGetLastError();
}

hipError_t mpdata_cell_add_ref(void* f, int elem_bytes, long long ld, long long sl0, long long n, int nx, int nlev, int ntr,
                               const void* s, double c, int clip, void* dsum, hipStream_t stream) {
  if (!f || !s || ld < 1 || sl0 < 0 || n < 1 || sl0 + n > ld || nx < 1 || nlev < 1 || ntr < 1 || (elem_bytes != 4 && elem_bytes != 8))
    return hipErrorInvalidValue;
  const long long rows = (long long)nlev * ntr;
  dim3 grid;
  if (ref_block_grid(n, rows, &grid) != hipSuccess) return hipErrorInvalidValue;
  return ref_real(elem_bytes, [&](auto r) {
    typedef decltype(r) R;
    hipLaunchKernelGGL((ref_cell_add_kernel<R>), grid, dim3(256), 0, stream, static_cast<R*>(f), ld, sl0, n, nx, rows,
                       static_cast<const R*>(s), c, clip, static_cast<R*>(dsum));
    return hipGetLastError();
  });
}
