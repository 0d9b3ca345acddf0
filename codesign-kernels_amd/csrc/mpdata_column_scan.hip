// mpdata_column_scan.hip -- running column integral of one tracer of f into another, in place (include/mpdata_hip.h 3aa,
// mpdata_column_scan.h): o(k) = the sum of wgt * f(src) from the surface up to level k, or from the top down to it, stored
// into tracer dst at every level, and the final sum per column.  One pass: a source and a destination tracer, no factor
// kernel in front.  Kernels of their own outside the run: nothing is fused into the plan kernels, nothing is kept between
// calls.
//   plan layout: the geometry of mpdata_vsolve.hip.  A workgroup takes UG adjacent units (8-byte elements of the instance
//     axis) and CB columns: its four waves copy the column slots of src of the group's tiles as linear streams (lane ->
//     element of the chunk, NB columns in flight) into LDS, re-laid as [column][unit][level] with an odd level stride,
//     together with the weight row of the group's units; after a barrier a lane per (unit, column) sweeps its column in
//     LDS in place (o over f) and stores total; after a second barrier the waves store LDS to the slots of dst, which lie
//     at a signed 64-bit offset from those of src, as the same linear streams.  Direction and inclusion are uniform values
//     of the launch: the staging code exists once.
//     Race freedom: workgroups own disjoint (group, column batch) element sets of src AND of dst, nothing couples columns
//     or instances; inside a workgroup every global load of a stage (of src, and of the halves of dst that are stored back
//     as loaded) precedes a barrier and every global store follows the sweep's barrier; dst == src is the in-place form
//     of mpdata_vsolve.hip, with dst != src the source tracer is never written; idle lanes clamp their addresses and store
//     nothing, and no barrier sits under a condition that differs inside a workgroup.
//     A windowed plan: the workgroup walks the windows of its units upward (UP) or downward (DOWN) -- stages a window,
//     continues the sum with s carried in the lane's registers, stores o into the owned levels of dst: f is read once and
//     written once.  The halves of an fp32 element are then different windows, of one instance or of two, so the halves
//     are swept one after the other in the order of the walk.
//   reference layout: one thread per instance, coalesced along sl, the columns over grid.y; the thread owns its column.
// Built with -ffp-contract=off: every operation of the definition is rounded once, in its association.  No reduction
// and no scan across lanes: the sum of a column is sequential in k.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "mpdata_column_scan.h"

namespace {

using namespace wm_walk;

// (LDS_ELEMS, the LDS of a workgroup at most, and the column groups of the launch: mpdata_wm_walk.h)

// What the plan-layout kernel reads of the job and the geometry, in one compact argument (tile and unit indices fit an
// int: a plan has an int of tiles), as mpdata_vsolve.hip's.
struct CsArgs {
  const void* f;              // the plan side of tracer src
  long long doff;             // tracer dst from it, in 8-byte elements
  const void* wgt;            // NULL: rho * adz
  const void *rho, *adz;
  void* total;                // NULL: not wanted
  long long kc_tile_stride;
  long long n, sl0, ncrms;
  long long tile_stride;
  int t0, t1;                 // tiles the block touches
  int g0, ngroup;             // first group, groups
  int chunk, main_e, ncol_p, nlev, slp;
  int W, nz;
  int UG, CB, ncb, ns;        // ns: level stride in LDS (odd)
  int ush;                    // UG = 1 << ush
  int down, excl;
};

// The sweep of a lane over the levels [l0, l1) of its column in LDS, upward or downward, HN halves of the element in
// lockstep from half h0:  p = w(k) * v(k);  t = c + p;  v(k) = excl ? c : t;  c = t      c: the running s, carried
// NB levels of operands are read ahead of the chain.  on[j]: the half is written (else it keeps what was staged).
template <typename R2, int HN>
__device__ inline void sweep(R2* const v, const R2* const w, const int h0, const int l0, const int l1, const bool down, const bool excl,
                             typename Elem<R2>::R (&c)[HN], const bool (&on)[HN]) {
  typedef Elem<R2> E;
  typedef typename E::R R;
  constexpr int N = E::N;
  R* const vr = reinterpret_cast<R*>(v);
  for (int kb = 0; kb < l1 - l0; kb += NB) {
    R2 fv[NB], wv[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const int ku = min(kb + u, l1 - l0 - 1);
      const int kc = down ? l1 - 1 - ku : l0 + ku;
      fv[u] = v[kc];
      wv[u] = w[kc];
    }
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      if (kb + u < l1 - l0) {
        const int kc = down ? l1 - 1 - kb - u : l0 + kb + u;
#pragma unroll
        for (int jj = 0; jj < HN; ++jj) {
          const int h = HN == N ? jj : h0;
          const R p = E::get(wv[u], h) * E::get(fv[u], h);
          const R t = c[jj] + p;
          const R o = excl ? c[jj] : t;
          c[jj] = t;
          if (on[jj]) vr[kc * N + h] = o;
        }
      }
    }
  }
}

// A uniform value held in vector registers: the windowed kernels have more uniform values than scalar registers.
template <bool V>
__device__ inline long long in_vgpr(long long x) {
  if (V) asm volatile("" : "+v"(x));
  return x;
}
template <bool V>
__device__ inline int int_in_vgpr(int x) {
  if (V) asm volatile("" : "+v"(x));
  return x;
}
template <typename T>
__device__ inline T* ptr_in_vgpr(T* x) {
  asm volatile("" : "+v"(x));
  return x;
}

// Plan layout.  blockIdx.x = group * ncb + column batch; R2: one 8-byte element (double, or the float2 of two adjacent
// slots); WIN: a windowed plan (W > 1, one slot per tile).
template <typename R2, bool WIN>
__global__ void __launch_bounds__(256) wm_column_scan_kernel(const CsArgs g) {
  typedef Elem<R2> E;
  typedef typename E::R R;
  constexpr int N = E::N;
  extern __shared__ __align__(8) unsigned char cs_lds[];
  const int tid0 = threadIdx.x;
  const int cb = blockIdx.x % g.ncb;
  const int gi = blockIdx.x / g.ncb;
  const int nlev = g.nlev, nx = g.ncol_p - 6, slp = WIN ? 1 : g.slp, W = WIN ? g.W : 1, ns = g.ns, UG = g.UG;
  const int nzm = int_in_vgpr<WIN>(g.nz - 1), t0 = int_in_vgpr<WIN>(g.t0), t1 = int_in_vgpr<WIN>(g.t1);
  const int main_e = int_in_vgpr<WIN>(g.main_e), ncol_p = int_in_vgpr<WIN>(g.ncol_p);
  const bool down = g.down != 0, excl = g.excl != 0;
  const long long n = in_vgpr<WIN>(g.n), sl0 = in_vgpr<WIN>(g.sl0), tile_stride = in_vgpr<WIN>(g.tile_stride);
  const long long doff = in_vgpr<true>(g.doff), kc_tile_stride = in_vgpr<true>(g.kc_tile_stride);   // (every kind of plan: the
  R* const total = ptr_in_vgpr(static_cast<R*>(g.total));                                            //  call has more uniform values than 3o)
  const int c0 = int_in_vgpr<WIN>(cb * g.CB), cbn = min(g.CB, nx - cb * g.CB);
  const int ue0 = int_in_vgpr<WIN>((g.g0 + gi) * UG);
  const int tile0 = WIN ? ue0 : ue0 / slp;
  const int ntg = WIN ? UG : UG / slp;
  const int nslice = WIN ? 1 : (g.chunk + 63) / 64;   // (a window is 63 levels at most)
  const int rem_e = g.chunk - main_e;
  R2* const lf = reinterpret_cast<R2*>(cs_lds);   // [column][unit][ns]: f of src, then o
  R2* const lw = lf + g.CB * UG * ns;             // [unit][ns]: the weights
  const R2* const f = ptr_in_vgpr(static_cast<const R2*>(g.f));
  const R* const gw = ptr_in_vgpr(static_cast<const R*>(g.wgt));
  const R2* const grho = ptr_in_vgpr(static_cast<const R2*>(g.rho));
  const R2* const gadz = ptr_in_vgpr(static_cast<const R2*>(g.adz));
  R carry[N];   // per instance of the unit: the running s
#pragma unroll
  for (int a = 0; a < N; ++a) carry[a] = 0;
  // a windowed plan: the constants of the windows the halves of the W tiles of a unit are, once, through LDS (read back
  // per lane: held by the scalar unit, the window arithmetic and its 64-bit divide spill scalar registers)
  int* const lwin = reinterpret_cast<int*>(lw + UG * ns);   // [tile of the unit][half]{k0, first owned, last owned + 1, instance of the unit}
  if (WIN) {
    const int tid = tid0;
    if (tid < W * N) {
      int k0 = 0, nz_w, own0 = 1, own1 = 0;
      if (mpd_level_window(g.nz, tid % W, &k0, &nz_w, &own0, &own1) != W) own1 = own0 - 1;
      lwin[4 * tid] = k0; lwin[4 * tid + 1] = own0 - 1 - k0; lwin[4 * tid + 2] = max(own1 - k0, own0 - 1 - k0); lwin[4 * tid + 3] = tid / W;
    }
    __syncthreads();
  }

  for (int mi = 0; mi < W; ++mi) {
    const int m = down ? W - 1 - mi : mi;
    // the thread's places are formed anew per window (mpdata_vsolve.hip: what the compiler could hoist out of this loop
    // is more than the scalar unit has to spare)
    int tid = tid0;
    if (WIN) asm volatile("" : "+v"(tid));
    const int lane = tid & 63, wave = tid >> 6;
    const int ci = tid >> g.ush, ug = tid & (UG - 1);   // the lane's pair in the sweep
    const bool act = ci < cbn;
    const int ue = ue0 + ug;
    if (mi) __syncthreads();   // the stores of the window before are through with LDS
    // per half of tile (unit, m): slot q = (unit * W + m) * N + h is window q % W of instance unit * N + dih; its owned
    // levels are [l0h, l1h) of the chunk, level kk of it the tall level k0h + kk (a plain plan: all of them, k0h = 0)
    int k0h[N], l0h[N], l1h[N], dih[N];
#pragma unroll
    for (int h = 0; h < N; ++h) {
      k0h[h] = 0; l0h[h] = 0; l1h[h] = nlev; dih[h] = h;
      if (WIN) {
        const int* const wc = lwin + 4 * (m * N + h);
        k0h[h] = wc[0]; l0h[h] = wc[1]; l1h[h] = wc[2]; dih[h] = wc[3];
      }
    }
    // ---- stage src (store = false) or store to dst (store = true): a wave per tile of the group, lane -> element of the
    // chunk.  An element goes through LDS when one of its halves is a slot of the block (of a window: an owned level); a
    // half of it that the call does not write is staged from dst, where it returns.
    auto copy = [&](const bool store) {
      for (int tg = wave; tg < ntg; tg += 4) {
        const int tile = (tile0 + tg) * W + m;
        if (tile < t0 || tile > t1) continue;
        int lo = 0, hi = g.chunk;
        if (WIN) {
          lo = nlev; hi = 0;
#pragma unroll
          for (int h = 0; h < N; ++h) {
            const long long sl = (long long)(tile0 + tg) * N + dih[h];
            if (sl >= sl0 && sl < sl0 + n && l1h[h] > l0h[h]) { lo = min(lo, l0h[h]); hi = max(hi, l1h[h]); }
          }
          if (hi <= lo) continue;
        }
        const R2* const src = f + (long long)tile * tile_stride;
        for (int sc = 0; sc < nslice; ++sc) {
          const int e0 = sc * 64 + lane;
          bool in = e0 >= lo && e0 < hi;
          const int e = in ? e0 : lo;   // (idle lanes read an element that is read anyway and store nothing)
          const int es = WIN ? 0 : e / nlev, ek = e - es * nlev;   // (a window: one slot per tile)
          bool wr[N];   // the halves of the element the call writes
#pragma unroll
          for (int h = 0; h < N; ++h) {
            const long long sl = WIN ? (long long)(tile0 + tg) * N + dih[h] : ((long long)tile * slp + es) * N + h;
            wr[h] = sl >= sl0 && sl < sl0 + n && (!WIN || (e >= l0h[h] && e < l1h[h]));
          }
          if (!WIN) in = in && (wr[0] || wr[N - 1]);
          const bool mg = N == 2 && in && doff != 0 && !(wr[0] && wr[N - 1]);
          const bool in_main = e < main_e;
          const long long cstep = in_main ? main_e : rem_e;
          const R2* const p = src + (in_main ? e : (long long)ncol_p * main_e + (e - main_e)) + (3 + c0) * cstep;   // column 1 = slot 3
          R2* const q = const_cast<R2*>(p) + doff;   // the same place of dst
          R2* const d = lf + (long long)(tg * slp + es) * ns + ek;
          for (int i = 0; i < cbn; i += NB) {
            if (!store) {
              R2 v[NB];
#pragma unroll
              for (int u = 0; u < NB; ++u) v[u] = p[(long long)min(i + u, cbn - 1) * cstep];
              if (N == 2 && mg) {
                R2 dv[NB];
#pragma unroll
                for (int u = 0; u < NB; ++u) dv[u] = q[(long long)min(i + u, cbn - 1) * cstep];
#pragma unroll
                for (int u = 0; u < NB; ++u) {
#pragma unroll
                  for (int h = 0; h < N; ++h)
                    if (!wr[h]) E::at(v[u], h) = E::get(dv[u], h);
                }
              }
#pragma unroll
              for (int u = 0; u < NB; ++u)
                if (in && i + u < cbn) d[(long long)(i + u) * UG * ns] = v[u];
            } else {
              R2 v[NB];
#pragma unroll
              for (int u = 0; u < NB; ++u) v[u] = d[(long long)min(i + u, cbn - 1) * UG * ns];
#pragma unroll
              for (int u = 0; u < NB; ++u)
                if (in && i + u < cbn) q[(long long)(i + u) * cstep] = v[u];
            }
          }
        }
      }
    };
    copy(false);
    // the weights of the group's units.  wgt: by tall level, the unit fastest (adjacent lanes read adjacent instances), a
    // half outside the block takes +0.  NULL: rho * adz of the slot where they lie, one rounded multiply, the level fastest.
    if (gw) {
      for (int x = tid; x < UG * nlev; x += 256) {
        const int kk = x >> g.ush, u2 = x & (UG - 1);
        R2 w2;
#pragma unroll
        for (int h = 0; h < N; ++h) {
          const long long sl = (long long)(ue0 + u2) * N + dih[h];
          const int kt = k0h[h] + kk;
          R wv = 0;
          if (sl >= sl0 && sl < sl0 + n && kt < nzm) wv = gw[(sl - sl0) + n * kt];
          E::at(w2, h) = wv;
        }
        lw[u2 * ns + kk] = w2;
      }
    } else {
      for (int x = tid; x < UG * nlev; x += 256) {
        const int u2 = x / nlev, kk = x - u2 * nlev;
        const int ue2 = ue0 + u2;
        const int tile = WIN ? ue2 * W + m : ue2 / slp;
        R2 w2;
#pragma unroll
        for (int h = 0; h < N; ++h) E::at(w2, h) = 0;
        if (tile >= t0 && tile <= t1) {
          const long long o = (long long)tile * kc_tile_stride + (long long)(ue2 % slp) * nlev + kk;
          const R2 r2 = grho[o], a2 = gadz[o];
#pragma unroll
          for (int h = 0; h < N; ++h) E::at(w2, h) = E::get(r2, h) * E::get(a2, h);
        }
        lw[u2 * ns + kk] = w2;
      }
    }
    __syncthreads();
    // ---- the sweep: a lane per (unit, column)
    if (act) {
      R2* const pf = lf + ((long long)ci * UG + ug) * ns;
      const R2* const pw = lw + ug * ns;
      if (!WIN) {
        bool on[N], any = false;
#pragma unroll
        for (int h = 0; h < N; ++h) {
          const long long sl = (long long)ue * N + h;
          on[h] = sl >= sl0 && sl < sl0 + n;
          any = any || on[h];
        }
        if (any) {
          sweep<R2, N>(pf, pw, 0, 0, nlev, down, excl, carry, on);
          // the phantom half follows the plan's last instance, its partner in the pair
          if (N == 2 && (g.ncrms & 1) && (long long)ue * N + 1 == g.ncrms && on[0]) {
            for (int k = 0; k < nlev; ++k) {
              R2 v = pf[k];
              E::at(v, N - 1) = E::get(v, 0);
              pf[k] = v;
            }
          }
          if (total) {
#pragma unroll
            for (int h = 0; h < N; ++h)
              if (on[h]) total[((long long)ue * N + h - sl0) + n * (c0 + ci)] = carry[h];
          }
        }
      } else {
        const int tile = ue * W + m;
#pragma unroll
        for (int hh = 0; hh < N; ++hh) {
          const int h = down ? N - 1 - hh : hh;   // downward: the higher slot first
          const int di1 = h ? dih[N - 1] : dih[0], l0 = h ? l0h[N - 1] : l0h[0], l1 = h ? l1h[N - 1] : l1h[0];   // (selects, no indexing)
          const long long sl = (long long)ue * N + di1;
          const bool on1[1] = {tile >= t0 && tile <= t1 && sl >= sl0 && sl < sl0 + n && l1 > l0};
          if (on1[0]) {
            R c1[1] = {di1 ? carry[N - 1] : carry[0]};
            sweep<R2, 1>(pf, pw, h, l0, l1, down, excl, c1, on1);
            if (di1) carry[N - 1] = c1[0]; else carry[0] = c1[0];
          }
        }
        // behind the last window of the walk the lane holds the final s of its instances
        if (mi == W - 1 && total) {
#pragma unroll
          for (int a = 0; a < N; ++a) {
            const long long sl = (long long)ue * N + a;
            if (sl >= sl0 && sl < sl0 + n) total[(sl - sl0) + n * (c0 + ci)] = carry[a];
          }
        }
      }
    }
    __syncthreads();
    copy(true);
  }
}

// Reference layout: element (sl, column i, level k, tracer t) at f + sl + ld * ((i + 2) + (nx + 6) * ((k - 1) + nlev * t)).
// x: instances of the block, y: columns i - 1.  wgt (n, nlev), or rho and adz at sl + ld * (k - 1).
template <typename R>
__global__ void __launch_bounds__(256) ref_column_scan_kernel(R* f, const long long doff, const R* __restrict__ wgt, const R* __restrict__ rho,
                                                             const R* __restrict__ adz, const long long ld, const long long sl0,
                                                             const long long n, const int nx, const int nlev, const int down,
                                                             const int excl, R* __restrict__ total) {
  const long long bi = (long long)blockIdx.x * 256 + threadIdx.x;
  if (bi >= n) return;
  const long long sl = sl0 + bi, step = ld * (nx + 6);
  for (long long i = blockIdx.y; i < nx; i += gridDim.y) {
    const R* const q = f + sl + ld * (i + 3);
    R* const o = f + doff + sl + ld * (i + 3);
    R c = 0;
    for (int k = 0; k < nlev; k += NB) {
      R v[NB], w[NB];
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        const long long ku = min(k + u, nlev - 1);
        const long long kc = down ? nlev - 1 - ku : ku;
        v[u] = q[kc * step];
        if (wgt) {
          w[u] = wgt[bi + n * kc];
        } else {
          const R rv = rho[sl + ld * kc], av = adz[sl + ld * kc];
          w[u] = rv * av;
        }
      }
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        if (k + u < nlev) {
          const long long kc = down ? nlev - 1 - k - u : k + u;
          const R p = w[u] * v[u];
          const R t = c + p;
          o[kc * step] = excl ? c : t;
          c = t;
        }
      }
    }
    if (total) total[bi + n * i] = c;
  }
}

}  // namespace

hipError_t mpdata_column_scan_wm(const MpdataColumnScanJob& b, hipStream_t stream) {
  WmGrid wg;
  const MpdataLayoutJob& j = b.j;
  if (j.ntr != 1 || j.prv_col0 != 0 || j.ncols != j.ncol_p) return hipErrorInvalidValue;
  if (!b.wgt && (!b.rho || !b.adz || b.kc_tile_stride < j.chunk)) return hipErrorInvalidValue;
  if (b.mode & ~(MPDATA_COLUMN_SCAN_MODE_DOWN | MPDATA_COLUMN_SCAN_MODE_EXCLUSIVE)) return hipErrorInvalidValue;
  const hipError_t e = wm_block_grid(j, b.sel, 1, &wg);
  if (e != hipSuccess) return e;
  const int W = b.sel.W;
  CsArgs g;
  g.f = j.prv; g.doff = b.doff; g.wgt = b.wgt; g.rho = b.rho; g.adz = b.adz; g.total = b.total;
  g.kc_tile_stride = b.kc_tile_stride;
  g.n = b.sel.n; g.sl0 = b.sel.sl0; g.ncrms = b.sel.ncrms;
  g.tile_stride = j.prv_tile_stride;
  g.t0 = (int)wg.t0; g.t1 = (int)(wg.t0 + wg.ntile - 1);
  g.chunk = (int)j.chunk; g.main_e = (int)j.main_e; g.ncol_p = j.ncol_p; g.nlev = j.nlev; g.slp = j.slp;
  g.W = W; g.nz = b.sel.nz;
  g.down = (b.mode & MPDATA_COLUMN_SCAN_MODE_DOWN) != 0; g.excl = (b.mode & MPDATA_COLUMN_SCAN_MODE_EXCLUSIVE) != 0;
  if (W > 128 || (W > 1 && j.chunk > 64)) return hipErrorInvalidValue;   // (the window table: a thread per slot of a unit; nz < 7000)
  const int win_e = W > 1 ? 2 * W * b.sel.ipe : 0;   // the window table: 16 bytes per slot of a unit
  // the weight row next to the columns; the kernel forms the tiles of a windowed plan from units, in int
  ColGroups cg;
  if (j.chunk > 2147483647LL || j.main_e > 2147483647LL ||
      !col_groups_batched(j, b.sel, wg, LDS_ELEMS, /*fixed*/ win_e, /*rows*/ 1, /*unit_mul*/ W, &cg))
    return hipErrorInvalidValue;
  col_groups_fill(cg, &g);
  g.ncb = cg.ncb; g.ush = cg.ush;
  const unsigned blocks = (unsigned)(cg.ngroup * g.ncb);
  const size_t lds = (size_t)cg.lds_e * 8;
  void (*k)(CsArgs) = b.sel.ipe == 1 ? (W > 1 ? wm_column_scan_kernel<double, true> : wm_column_scan_kernel<double, false>)
                                     : (W > 1 ? wm_column_scan_kernel<float2, true> : wm_column_scan_kernel<float2, false>);
  hipLaunchKernelGGL(k, dim3(blocks), dim3(256), lds, stream, g);
  return hipGetLastError();
}

hipError_t mpdata_column_scan_ref(void* f, int elem_bytes, long long ld, long long sl0, long long n, int nx, int nlev, int ntr, int src,
                                  int dst, const void* wgt, const void* rho, const void* adz, void* total, int mode, hipStream_t stream) {
  if (!f || (!wgt && (!rho || !adz)) || ld < 1 || sl0 < 0 || n < 1 || sl0 + n > ld || nx < 1 || nlev < 1 || ntr < 1 || src < 0 ||
      src >= ntr || dst < 0 || dst >= ntr || (elem_bytes != 4 && elem_bytes != 8) ||
      (mode & ~(MPDATA_COLUMN_SCAN_MODE_DOWN | MPDATA_COLUMN_SCAN_MODE_EXCLUSIVE)))
    return hipErrorInvalidValue;
  dim3 grid;
  if (ref_block_grid(n, nx, &grid) != hipSuccess) return hipErrorInvalidValue;
  const long long tstep = ld * (nx + 6) * nlev;
  return ref_real(elem_bytes, [&](auto r) {
    typedef decltype(r) R;
    hipLaunchKernelGGL((ref_column_scan_kernel<R>), grid, dim3(256), 0, stream, static_cast<R*>(f) + tstep * src, tstep * (dst - src),
                       static_cast<const R*>(wgt), static_cast<const R*>(rho), static_cast<const R*>(adz), ld, sl0, n, nx, nlev,
                       (mode & MPDATA_COLUMN_SCAN_MODE_DOWN) != 0, (mode & MPDATA_COLUMN_SCAN_MODE_EXCLUSIVE) != 0, static_cast<R*>(total));
    return hipGetLastError();
  });
}
