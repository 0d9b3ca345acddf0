// mpdata_sediment.hip -- sedimentation of f, in place (include/mpdata_hip.h 3n, mpdata_sediment.h): precipitating water
// falling along k with a fall coefficient wp that differs in every cell and tracer (SAM's precip_fall), a Jacobi update
// of the interior columns from the downward fluxes Fz = wp * f of the OLD field.  The first block call that reads a
// per-cell field in the reference layout where it lies.  A kernel of its own outside the run: nothing is fused into the
// plan kernels, nothing is kept between calls.
//   plan layout: a workgroup owns the whole tiles of a GROUP of UG adjacent 8-byte elements of the instance axis (units:
//     an instance, or a pair of an fp32 plan).  f is walked as mpdata_subside.hip walks it -- a wave per 64-element slice
//     of a tile's column chunk, lane -> element e = s * nlev + kk, the interior column slots 3 .. nx+2 as linear streams
//     with the main / rest split, up to NB columns in flight -- but a wave visits the tiles of its group in ROUNDS of
//     4 / nslice tiles.  Per batch of CB columns:
//       (A) barrier; the four waves copy the group's rows of wp -- UG units wide, whole 128-byte lines of an aligned
//           whole-plan call -- into LDS as [column][unit][level] with an odd level stride (the first batch: 1 / (rho *
//           adz) of the group's slots too);
//       per round: every load of f -- the lane's own element and, above 64 levels, the element above lane 63 in the
//           slice next door -- then (B) barrier, then the LDS reads and every store of the round.
//     Fz(k+1) of a lane is the product lane kk + 1 forms, by shuffle: same operands, same bits; the top level takes +0;
//     lane 63 forms it from the edge load and that element's wp in LDS.  Race freedom: DESIGN.md 4.17.
//     A windowed plan: a workgroup per group AND window (blockIdx.y) -- a window reads and writes its own tile only --,
//     each staged by tall level from the caller's wp.  psfc is written by a small kernel of its own in front, while f
//     is the old field (wm_sediment_psfc_kernel), so the hot kernel carries neither its pointer nor its predicate.
//     The running sums of pflux live in LDS, one slot per (round, thread), touched by that thread alone.
//   reference layout: one thread per instance and (level, tracer) row, coalesced along sl.  pflux is a sum over i in
//     rising order, so a thread marches a row; row k + 1 belongs to a thread of another workgroup, so the new interior
//     goes to a scratch array and a second kernel on the same stream copies it into f: the kernel boundary is the order.
// Built with -ffp-contract=off and IEEE divides: every operation of the definition is rounded once, in its association.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "mpdata_sediment.h"

namespace {

using namespace wm_walk;

// (LDS_ELEMS, the LDS of a workgroup at most, and the column groups of the launch: mpdata_wm_walk.h)

__device__ inline double lane_down(const double v) { return __shfl_down(v, 1); }  // the value of lane + 1
__device__ inline float2 lane_down(const float2 v) { return make_float2(__shfl_down(v.x, 1), __shfl_down(v.y, 1)); }

// Per-lane conditions that live across a round -- the half is in the block, its level has one above, the half is the
// phantom -- are kept as bit masks in vector registers (all ones / zero) and applied to the bit patterns: held as lane
// masks they would take two scalar registers each, and the kernel has more of them than scalar registers to spare.  The
// empty asm keeps the compiler from turning the masks back into lane masks; the selections are exact (no arithmetic).
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

// The workgroups of the plan-layout kernel.  A UNIT is one 8-byte element of the instance axis: slot ue % slp of tile
// ue / slp, or, in a windowed plan, the tiles ue * W .. ue * W + W - 1.  A workgroup takes UG adjacent units (a multiple
// of slp) and walks the columns in batches of CB.  The kernel takes what it reads of the job and the geometry in one
// compact argument (tile and unit indices fit an int: a plan has an int of tiles): fewer scalar registers than the job.
struct SedArgs {
  void* f;                    // the plan side of f, first tracer of the call
  const void *wp, *rho, *adz;
  void *psfc, *pflux;
  long long n, sl0, nslots;   // the block; the plan's slots (ncrms * W)
  long long tstride, tile_stride, kc_tile_stride;
  int chunk, main_e, ncol_p, nlev, slp;
  int W, nz;
  int t0, t1;                 // tiles the block touches
  int g0, ngroup;             // first group, groups
  int UG, CB, ns;             // ns: level stride in LDS (odd)
  int ush;                    // UG = 1 << ush
  int nslice, nround;
};

// Plan layout.  blockIdx.x = tracer * ngroup + group; R2: one 8-byte element (double, or the float2 of two adjacent slots);
// WIN: a windowed plan (W > 1, one slot per tile) -- the plain plans carry no window constants and no loop over windows;
// a workgroup per window (blockIdx.y), the constants of its halves' windows in LDS behind the running sums.  PAIRS: wp is staged
// in whole 8-byte elements (fp64; an fp32 block whose pairs are whole and 8-byte aligned in wp), else in single reals.
template <typename R2, bool WIN, bool PAIRS>
__global__ void __launch_bounds__(256) wm_sediment_kernel(const SedArgs g) {
  typedef Elem<R2> E;
  typedef typename E::R R;
  constexpr int N = E::N;
  extern __shared__ __align__(8) unsigned char sed_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int gi = blockIdx.x % g.ngroup;
  const int tr = blockIdx.x / g.ngroup;
  const int nlev = g.nlev, nx = g.ncol_p - 6, slp = WIN ? 1 : g.slp, W = WIN ? g.W : 1, ns = g.ns, UG = g.UG;
  const int nslice = g.nslice, tpw = 4 / nslice, ntg = UG / slp;
  const int nzm = g.nz - 1;
  const long long n = g.n, sl0 = g.sl0;
  const int ue0 = (g.g0 + gi) * UG;
  R2* const lw = reinterpret_cast<R2*>(sed_lds);    // [column][unit][ns]: wp
  R2* const lir = lw + g.CB * UG * ns;              // [unit][ns]: 1 / (rho * adz)
  R2* const lacc = lir + UG * ns;                   // [round][thread]: the running sums of pflux
  int* const lwin = reinterpret_cast<int*>(lacc + g.nround * 256);   // WIN: [half]{k0, own0, own1, -}
  R2* const f = static_cast<R2*>(g.f) + (long long)tr * g.tstride;
  const R* const wp = static_cast<const R*>(g.wp) + n * ((long long)nx * nzm * tr);

  // the lane's element of a chunk (the same in every tile the wave visits) and its neighbour above in the next slice
  const bool wave_in = wave < tpw * nslice;   // (three slices: the fourth wave idles)
  const int slice = wave % nslice;
  const int e0 = slice * 64 + lane;
  const bool lane_in = wave_in && e0 < g.chunk;
  const int e = lane_in ? e0 : 0;   // (idle lanes read element 0 and store nothing)
  const int s = e / nlev, kk = e - s * nlev;
  const bool edge = lane_in && lane == 63 && kk + 1 < nlev;   // (then e + 1 is a level of the same slot)
  const int ee = edge ? e + 1 : e;
  const int rem_e = g.chunk - g.main_e;
  const bool main_o = e < g.main_e, main_e = ee < g.main_e;
  const int so = main_o ? g.main_e : rem_e, se = main_e ? g.main_e : rem_e;   // column strides
  const int oo = main_o ? e : g.ncol_p * g.main_e + (e - g.main_e);
  const int oe = main_e ? ee : g.ncol_p * g.main_e + (ee - g.main_e);

  // a windowed plan: blockIdx.y is the tile m of every unit of the group -- a window reads and writes its own tile only, so
  // the W tiles of a unit are as independent as units are; the constants of its (two) windows go through LDS
  const int m = WIN ? blockIdx.y : 0;
  if (WIN) {
    if (tid < N) {
      int k0 = 0, nz_w, own0 = 1, own1 = 0;
      if (mpd_level_window(g.nz, (m * N + tid) % W, &k0, &nz_w, &own0, &own1) != W) own1 = own0 - 1;
      lwin[4 * tid] = k0; lwin[4 * tid + 1] = own0; lwin[4 * tid + 2] = own1;
    }
    __syncthreads();
  }
  {
    // the window each half of tile (unit, m) is: slot q = (unit * W + m) * N + h is window q % W of instance q / W
    int k0h[N], own0h[N], own1h[N], dih[N];
#pragma unroll
    for (int h = 0; h < N; ++h) {
      k0h[h] = 0; own0h[h] = 1; own1h[h] = nzm;
      dih[h] = h;
      if (WIN) {
        dih[h] = (m * N + h) / W;
        k0h[h] = lwin[4 * h]; own0h[h] = lwin[4 * h + 1]; own1h[h] = lwin[4 * h + 2];
      }
    }
    for (int c0 = 0; c0 < nx; c0 += g.CB) {
      const int cbn = min(g.CB, nx - c0);
      __syncthreads();   // (A) every wave is through with the LDS of the batch before
      if (c0 == 0) {
        // 1 / (rho * adz) of the group's slots: one rounded multiply, one IEEE divide
        for (int x = tid; x < UG * nlev; x += 256) {
          const int u2 = x / nlev, k2 = x - u2 * nlev;
          const int ue2 = ue0 + u2;
          const int tile = ue2 / slp * W + m;
          R2 q2;
#pragma unroll
          for (int h = 0; h < N; ++h) E::at(q2, h) = 0;
          if (tile >= g.t0 && tile <= g.t1) {
            const long long o = tile * g.kc_tile_stride + (ue2 % slp) * nlev + k2;
            const R2 r2 = static_cast<const R2*>(g.rho)[o], a2 = static_cast<const R2*>(g.adz)[o];
#pragma unroll
            for (int h = 0; h < N; ++h) E::at(q2, h) = (R)1 / (E::get(r2, h) * E::get(a2, h));
          }
          lir[u2 * ns + k2] = q2;
        }
      }
      // ---- stage wp: a row of the group is UG units, adjacent in wp wherever the slots are adjacent instances (a row
      // is a power of two of elements, 256 at most: a thread keeps its place in the row)
      if (PAIRS) {
        // whole 8-byte elements: fp64, or an fp32 block whose pairs are whole and 8-byte aligned in wp
        const int u2 = tid & (UG - 1);
        const long long sl = (long long)(ue0 + u2) * N;
        const bool in = sl >= sl0 && sl + N <= sl0 + n;
        const R2* const src = reinterpret_cast<const R2*>(wp + (in ? sl - sl0 : 0));
        const long long n2 = n / N;
        for (int row = tid >> g.ush; row < cbn * nlev; row += 256 >> g.ush) {
          const int ci = row / nlev, k2 = row - ci * nlev;
          R2 v;
#pragma unroll
          for (int h = 0; h < N; ++h) E::at(v, h) = 0;
          if (in && k0h[0] + k2 < nzm) v = src[n2 * ((c0 + ci) + (long long)nx * (k0h[0] + k2))];
          lw[(ci * UG + u2) * ns + k2] = v;
        }
      } else {
        const int inst = tid & (N * UG - 1), u2 = inst / N, h = inst - u2 * N;
        const long long sl = (long long)(ue0 + u2) * N + (h ? dih[N - 1] : dih[0]);
        const int k0 = h ? k0h[N - 1] : k0h[0];
        const int rsh = g.ush + (N - 1);
        const bool in = sl >= sl0 && sl < sl0 + n;
        const R* const src = wp + (in ? sl - sl0 : 0);
        for (int row = tid >> rsh; row < cbn * nlev; row += 256 >> rsh) {
          const int ci = row / nlev, k2 = row - ci * nlev;
          const int kt = k0 + k2;
          R v = 0;
          if (in && kt < nzm) v = src[n * ((c0 + ci) + (long long)nx * kt)];
          reinterpret_cast<R*>(lw)[((ci * UG + u2) * ns + k2) * N + h] = v;
        }
      }
      for (int r = 0; r < g.nround; ++r) {
        const int tg = r * tpw + wave / nslice;
        const int tile_r = (ue0 / slp + tg) * W + m;
        const bool task = wave_in && tg < ntg && tile_r >= g.t0 && tile_r <= g.t1;
        const int tile = task ? tile_r : g.t0;   // (an idle wave reads tile t0 and stores nothing)
        const int ug = tg < ntg ? tg * slp + s : 0;
        // per half: the instance and the tall level the slot stands for
        int onm[N], upm[N], phm[N];
        long long bi[N];
        int kt[N];
        bool any = false;
#pragma unroll
        for (int h = 0; h < N; ++h) {
          const long long q = ((long long)tile * slp + s) * N + h;
          const bool ph = N == 2 && (g.nslots & 1) && q == g.nslots;   // the phantom half follows the plan's last slot
          const int hq = ph ? 0 : h;   // (unrolled: a constant index or a select)
          const long long sl = WIN ? (long long)(ue0 + tg) * N + dih[hq] : (ph ? q - 1 : q);   // = (ph ? q - 1 : q) / W
          kt[h] = k0h[hq] + kk;
          upm[h] = vmask(kt[h] + 1 < nzm);   // else the top level: Fz(k+1) = +0
          bool ok = task && lane_in && sl >= sl0 && sl < sl0 + n && kt[h] < nzm;
          if (WIN) ok = ok && kt[h] + 1 >= own0h[hq] && kt[h] + 1 <= own1h[hq];
          onm[h] = vmask(ok);   // else: padding, the partner of a split pair, a neighbour in the group, a level the window does not own
          phm[h] = vmask(ph);
          any = any || ok;
          bi[h] = ok ? sl - sl0 : 0;
        }
        const bool wave_any = __ballot(any) != 0;
        R2* const pf = f + tile * g.tile_stride + oo + (3 + c0) * so;   // column c0 + 1 = slot c0 + 3
        const R2* const pfe = f + tile * g.tile_stride + oe + (3 + c0) * se;
        // ---- every load of f of the round (indices clamped, not predicated)
        R2 v[NB], fe[NB];
        {
          const R2* p = pf;
#pragma unroll
          for (int u = 0; u < NB; ++u) {
            v[u] = *p;
            if (u + 1 < cbn) p += so;
          }
          const R2* pe = pfe;
#pragma unroll
          for (int u = 0; u < NB; ++u) {
            fe[u] = v[u];
            if (edge) fe[u] = *pe;
            if (u + 1 < cbn) pe += se;
          }
        }
        __syncthreads();   // (B) every wave has loaded what this round's stores overwrite; wp and ir are in LDS
        if (wave_any) {
          const R2 ir2 = lir[ug * ns + kk];
          R2 acc;
#pragma unroll
          for (int h = 0; h < N; ++h) E::at(acc, h) = 0;
          if (g.pflux && c0 > 0) acc = lacc[r * 256 + tid];
          const int anym = onm[0] | onm[N - 1];
          const R2* pw = lw + ug * ns + kk;   // the lane's element of wp, a column per step
          R2* po = pf;
#pragma unroll
          for (int u = 0; u < NB; ++u) {
            if (u < cbn) {
              const R2 fcur = v[u];
              const R2 w2 = pw[0];
              R2 fz;
#pragma unroll
              for (int h = 0; h < N; ++h) E::at(fz, h) = E::get(w2, h) * E::get(fcur, h);
              R2 fzu = lane_down(fz);
              if (edge) {
                const R2 w2e = pw[1];
#pragma unroll
                for (int h = 0; h < N; ++h) E::at(fzu, h) = E::get(w2e, h) * E::get(fe[u], h);
              }
              R2 out = fcur;
#pragma unroll
              for (int h = 0; h < N; ++h) {
                const R f_c = E::get(fcur, h), fz_c = E::get(fz, h);
                const R fz_u = pick(E::get(fzu, h), (R)0, upm[h]);
                const R d = fz_c - fz_u;
                const R nv = f_c - d * E::get(ir2, h);
                E::at(acc, h) = E::get(acc, h) + fz_c;
                E::at(out, h) = pick(nv, f_c, onm[h]);
              }
              if (N == 2) E::at(out, N - 1) = pick(E::get(out, 0), E::get(out, N - 1), phm[N - 1] & onm[N - 1]);
              if (anym) *po = out;
              po += so;
              pw += UG * ns;
            }
          }
          if (g.pflux) {
            if (c0 + g.CB < nx) {
              lacc[r * 256 + tid] = acc;
            } else {
#pragma unroll
              for (int h = 0; h < N; ++h)
                if (onm[h] && !phm[h]) static_cast<R*>(g.pflux)[bi[h] + n * (kt[h] + (long long)nzm * tr)] = E::get(acc, h);
            }
          }
        }
      }
    }
  }
}

// What reaches the surface, psfc(b, i, t) = wp(b, i, 1, t) * f(i, 1): a kernel of its own IN FRONT of the one above, while
// f is the old field -- one level of 1 / nzm of the traffic, and the hot kernel keeps neither the pointer nor the
// predicate.  One thread per instance of the block (x) and column and tracer (y); tall level 1 is level 0 of window 0,
// slot q = sl * W, half q % N of element q / N.  The product has the operands of the hot kernel's Fz(i,1): the same bits.
template <typename R2>
__global__ void __launch_bounds__(256) wm_sediment_psfc_kernel(const SedArgs g, const int ntr) {
  typedef Elem<R2> E;
  typedef typename E::R R;
  constexpr int N = E::N;
  const long long bi = (long long)blockIdx.x * 256 + threadIdx.x;
  if (bi >= g.n) return;
  const int nx = g.ncol_p - 6, nzm = g.nz - 1;
  const long long q = (g.sl0 + bi) * g.W, el = q / N;
  const int h = (int)(q - el * N);
  const long long tile = el / g.slp;
  const int e = (int)(el - tile * g.slp) * g.nlev;   // level 0 of the slot
  const bool main_o = e < g.main_e;
  const long long so = main_o ? g.main_e : g.chunk - g.main_e;
  const long long oo = main_o ? e : (long long)g.ncol_p * g.main_e + (e - g.main_e);
  for (long long r = blockIdx.y; r < (long long)nx * ntr; r += gridDim.y) {
    const long long t = r / nx, i = r - t * nx;
    const R2 fv = static_cast<const R2*>(g.f)[t * g.tstride + tile * g.tile_stride + oo + (3 + i) * so];
    const R w = static_cast<const R*>(g.wp)[bi + g.n * (i + (long long)nx * nzm * t)];
    static_cast<R*>(g.psfc)[bi + g.n * r] = w * E::get(fv, h);
  }
}

// Reference layout: element (sl, column i, level k, tracer t) at f + sl + ld * ((i + 2) + (nx + 6) * ((k - 1) + nlev * t)), rho
// and adz at sl + ld * (k - 1), wp (b, i, k, t) at b + n * ((i - 1) + nx * ((k - 1) + nlev * t)).  x: instances of the block,
// y: rows r = (k - 1) + nlev * t.  The new interior goes to out (b, i - 1, r); f is only read.
template <typename R>
__global__ void __launch_bounds__(256) ref_sediment_kernel(const R* __restrict__ f, const R* __restrict__ rho, const R* __restrict__ adz,
                                                          const long long ld, const long long sl0, const long long n, const int nx,
                                                          const int nlev, const long long rows, const R* __restrict__ wp,
                                                          R* __restrict__ psfc, R* __restrict__ pflux, R* __restrict__ out) {
  const long long bi = (long long)blockIdx.x * 256 + threadIdx.x;
  if (bi >= n) return;
  const long long sl = sl0 + bi, lstep = ld * (nx + 6), wstep = n * nx;
  for (long long r = blockIdx.y; r < rows; r += gridDim.y) {
    const long long t = r / nlev;
    const int kk = (int)(r - t * nlev);
    const bool has_up = kk + 1 < nlev;
    const R* const p = f + sl + ld * (3 + (long long)(nx + 6) * r);   // column 1
    const R* const pw = wp + bi + wstep * r;
    const R* const pu = has_up ? p + lstep : p;
    const R* const pwu = has_up ? pw + wstep : pw;
    const R ir = (R)1 / (rho[sl + ld * kk] * adz[sl + ld * kk]);
    R* const o = out + bi + wstep * r;
    R acc = 0;
    for (int i = 0; i < nx; ++i) {
      const R fc = p[ld * i];
      const R fz = pw[n * i] * fc;
      const R fzu = has_up ? pwu[n * i] * pu[ld * i] : (R)0;
      const R d = fz - fzu;
      o[n * i] = fc - d * ir;
      acc = acc + fz;
      if (psfc && kk == 0) psfc[bi + n * (i + (long long)nx * t)] = fz;
    }
    if (pflux) pflux[bi + n * r] = acc;
  }
}
// ... and back: the interior columns of f := out
template <typename R>
__global__ void __launch_bounds__(256) ref_sediment_store_kernel(R* __restrict__ f, const long long ld, const long long sl0, const long long n,
                                                                const int nx, const long long rows, const R* __restrict__ out) {
  const long long bi = (long long)blockIdx.x * 256 + threadIdx.x;
  if (bi >= n) return;
  for (long long r = blockIdx.y; r < rows; r += gridDim.y) {
    R* const p = f + (sl0 + bi) + ld * (3 + (long long)(nx + 6) * r);   // column 1
    const R* const o = out + bi + n * ((long long)nx * r);
    for (int i = 0; i < nx; i += NB) {
      R v[NB];
#pragma unroll
      for (int u = 0; u < NB; ++u) v[u] = o[n * min(i + u, nx - 1)];
#pragma unroll
      for (int u = 0; u < NB; ++u)
        if (i + u < nx) p[ld * (i + u)] = v[u];
    }
  }
}

template <typename R>
hipError_t ref_launch(void* f, const void* rho, const void* adz, long long ld, long long sl0, long long n, int nx, int nlev, long long rows,
                      const void* wp, void* psfc, void* pflux, void* scratch, dim3 grid, hipStream_t stream) {
  hipLaunchKernelGGL((ref_sediment_kernel<R>), grid, dim3(256), 0, stream, static_cast<const R*>(f), static_cast<const R*>(rho),
                     static_cast<const R*>(adz), ld, sl0, n, nx, nlev, rows, static_cast<const R*>(wp), static_cast<R*>(psfc),
                     static_cast<R*>(pflux), static_cast<R*>(scratch));
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((ref_sediment_store_kernel<R>), grid, dim3(256), 0, stream, static_cast<R*>(f), ld, sl0, n, nx, rows,
                     static_cast<const R*>(scratch));
  return hipGetLastError();
}

}  // namespace

hipError_t mpdata_sediment_wm(const MpdataSedimentJob& b, hipStream_t stream) {
  WmGrid wg;
  const MpdataLayoutJob& j = b.j;
  if (!b.wp || !b.rho || !b.adz || j.prv_col0 != 0 || j.ncols != j.ncol_p || b.kc_tile_stride < j.chunk) return hipErrorInvalidValue;
  const hipError_t e = wm_block_grid(j, b.sel, j.ntr, &wg);
  if (e != hipSuccess) return e;
  // What follows holds for every plan mpdata_plan_create makes -- slp is 1, 2, 4 or 8, a chunk is 237 elements at most
  // (four slices), wm_block_grid has checked slp == 1 on a windowed plan -- so none of these returns is reached today; a
  // new tiling that breaks one of them must extend the kernel, and fails here, before any launch, until it does.
  // One buffer of wp, the row of quotients and the running sums, 32 units where a tile holds 8; fewer units where two
  // columns of the group's levels do not fit next to them.
  const int nx = j.ncol_p - 6, slp = j.slp, W = b.sel.W;
  ColGroups cg;
  // (unit, tile and slot-in-LDS arithmetic of the kernel is in int)
  if (!col_groups_tiled(j, b.sel, wg, LDS_ELEMS, /*fixed*/ W > 1 ? 4 : 0, /*rows*/ 1, /*bufs*/ 1, /*sums*/ true, /*wide*/ true,
                        &cg) ||
      (long long)j.ncol_p * j.main_e + j.chunk > 2147483647LL)
    return hipErrorInvalidValue;
  SedArgs g;
  g.f = j.prv; g.wp = b.wp; g.rho = b.rho; g.adz = b.adz; g.psfc = b.psfc; g.pflux = b.pflux;
  g.n = b.sel.n; g.sl0 = b.sel.sl0; g.nslots = b.sel.ncrms * W;
  g.tstride = j.prv_tstride; g.tile_stride = j.prv_tile_stride; g.kc_tile_stride = b.kc_tile_stride;
  g.chunk = (int)j.chunk; g.main_e = (int)j.main_e; g.ncol_p = j.ncol_p; g.nlev = j.nlev; g.slp = slp;
  g.W = W; g.nz = b.sel.nz;
  g.t0 = (int)wg.t0; g.t1 = (int)(wg.t0 + wg.ntile - 1);
  g.nslice = wg.nslice;
  col_groups_fill(cg, &g);
  g.ush = cg.ush; g.nround = cg.nround;
  // (W > 1: the halves of a pair are windows, not adjacent instances)
  const bool pairs = b.sel.ipe == 2 && W == 1 && b.sel.sl0 % 2 == 0 && b.sel.n % 2 == 0 && reinterpret_cast<uintptr_t>(b.wp) % 8 == 0;
  const size_t lds = (size_t)cg.lds_e * 8;
  void (*k)(SedArgs) = b.sel.ipe == 1 ? (W > 1 ? wm_sediment_kernel<double, true, true> : wm_sediment_kernel<double, false, true>)
                       : W > 1        ? wm_sediment_kernel<float2, true, false>
                       : pairs        ? wm_sediment_kernel<float2, false, true>
                                      : wm_sediment_kernel<float2, false, false>;
  if (b.psfc) {
    dim3 grid;
    if (ref_block_grid(b.sel.n, (long long)nx * j.ntr, &grid) != hipSuccess) return hipErrorInvalidValue;
    hipLaunchKernelGGL(b.sel.ipe == 1 ? wm_sediment_psfc_kernel<double> : wm_sediment_psfc_kernel<float2>, grid, dim3(256), 0, stream, g,
                       j.ntr);
    const hipError_t e2 = hipGetLastError();
    if (e2 != hipSuccess) return e2;
  }
  hipLaunchKernelGGL(k, dim3((unsigned)(g.ngroup * j.ntr), (unsigned)W), dim3(256), lds, stream, g);
  return hipGetLastError();
}

hipError_t mpdata_sediment_ref(void* f, const void* rho, const void* adz, int elem_bytes, long long ld, long long sl0, long long n,
                               int nx, int nlev, int ntr, const void* wp, void* psfc, void* pflux, void* scratch, hipStream_t stream) {
  if (!f || !rho || !adz || !wp || !scratch || ld < 1 || sl0 < 0 || n < 1 || sl0 + n > ld || nx < 1 || nlev < 1 || ntr < 1 ||
      (elem_bytes != 4 && elem_bytes != 8))
    return hipErrorInvalidValue;
  const long long rows = (long long)nlev * ntr;
  dim3 grid;
  if (ref_block_grid(n, rows, &grid) != hipSuccess) return hipErrorInvalidValue;
  return ref_real(elem_bytes, [&](auto r) {
    return ref_launch<decltype(r)>(f, rho, adz, ld, sl0, n, nx, nlev, rows, wp, psfc, pflux, scratch, grid, stream);
  });
}
