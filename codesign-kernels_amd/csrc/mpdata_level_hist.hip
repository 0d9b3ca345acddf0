// mpdata_level_hist.hip -- per-level histograms of the tracers of f (include/mpdata_hip.h 3ab, mpdata_level_hist.h): how
// many interior columns 1 .. nx of a level have the binned tracer inside each of nb bins (e_j, e_{j+1}], and the sum of every
// value tracer over exactly the columns of each bin -- the PDF of a tracer per level, a CFAD, tracer content binned by a
// conserved variable -- in ONE walk over the field for all bins.  A kernel of its own outside the run: nothing is fused
// into the plan kernels, nothing is kept between calls, nothing of the plan is written.
//   plan layout: the lane-owned walk of mpdata_level_cond.hip over the column slots 3 .. nx+2, NB columns in flight, the
//     value tracers at signed 64-bit offsets from the tc stream, a loop inside the kernel.  The edges are launch arguments.
//     The bins of a lane are registers: a compile-time array of the bin class under an unrolled select chain; a walk
//     carries at most 16 bins in fp64 and 8 in fp32, a call of more bins is a launch per group of bins (mpdata_level_hist.h).
//   reference layout: one thread per instance and level row, coalesced along sl, loops over i: the same walk.
// A column outside a bin is selected away, never multiplied away.  Built with -ffp-contract=off: every add is rounded once,
// in column order.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <limits>

#include "mpdata_level_hist.h"

namespace {

using namespace wm_walk;

constexpr int MAXB = MPDATA_LEVEL_HIST_BINS;

// bins a walk carries at most: the largest bin classes whose resource report shows no spill of either register file
// (the class of 32 spills scalar registers in both precisions, the class of 16 in fp32: DESIGN.md 4.31)
constexpr int GROUP_F64 = 16, GROUP_F32 = 8;

struct Edges {
  double e[MAXB + 1];
};

// m_i of one real: the number of the edges e[0 .. NE) that c exceeds (a NaN exceeds none)
template <typename R, int NE>
__device__ inline unsigned bin_m(const R c, const R (&e)[NE]) {
  unsigned m = 0;
#pragma unroll
  for (int j = 0; j < NE; ++j) m += c > e[j] ? 1u : 0u;
  return m;
}

// The REGISTERS walk over the columns p[0], p[step], ... of the binned tracer (and p[doff], p[doff + step], ... of the value
// tracer; !TWO: the binned tracer is the value), i ascending: CNT: q[j] = q[j] + 1, SUM: s[j] = s[j] + v_i for the one j with
// m_i == j + 1.  e: the NBC + 1 edges of the class, +inf behind nb, so that bin nb of a class that has one collects c_i >
// e_nb and is never stored.  All loads of a batch are issued before the first is used (the index is clamped, not
// predicated); the batch's tail is cut by wave-uniform conditions.  q and s are indexed by unrolled loops only.
template <typename R2, int NBC, bool CNT, bool SUM, bool TWO>
__device__ inline void march_hist(const R2* p, const long long doff, const long long step, const int nx,
                                  const typename Elem<R2>::R (&e)[NBC + 1], unsigned (&q)[Elem<R2>::N][NBC],
                                  typename Elem<R2>::R (&s)[Elem<R2>::N][NBC]) {
  typedef Elem<R2> E;
  typedef typename E::R R;
#pragma unroll
  for (int h = 0; h < E::N; ++h) {
#pragma unroll
    for (int j = 0; j < NBC; ++j) {
      if (CNT) q[h][j] = 0;
      if (SUM) s[h][j] = 0;
    }
  }
  const R2* const pv = p + doff;
#pragma nounroll
  for (int i = 0; i < nx; i += NB) {
    R2 vc[NB], vv[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) vc[u] = p[(long long)min(i + u, nx - 1) * step];
    if (SUM && TWO) {
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
          const unsigned m = bin_m<R, NBC + 1>(c, e);
#pragma unroll
          for (int j = 0; j < NBC; ++j) {
            const bool in = m == (unsigned)(j + 1);
            if (CNT) q[h][j] += in ? 1u : 0u;
            if (SUM) s[h][j] = in ? s[h][j] + v : s[h][j];
            // eight bins of a cell at a time: a compare mask is a scalar pair, and those of 32 bins, let alone of several
            // cells, do not fit the scalar file
            if (j % 8 == 7) __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
    }
  }
}

// what a lane of the plan-layout kernels owns: per half whether it is an output row of the block and where the row lies
template <int N>
struct Rows {
  bool in[N];
  long long o[N];
  bool any;
};

// lane -> element e = s * nlev + kk of (tile, slice) and its stream of tracer tc at column 1; false: the wave has no work
// (the twin of the head of wm_level_cond_kernel, mpdata_level_cond.hip: the same lanes, windows, pairs and block test -- a
// change to either belongs in both)
template <typename R2>
__device__ inline bool hist_rows(const MpdataLevelHistJob& b, const long long t0, const int ntile, const int nslice, const R2*& p,
                                 long long& cstep, Rows<Elem<R2>::N>& r) {
  typedef Elem<R2> E;
  const MpdataLayoutJob& j = b.j;
  const int lane = threadIdx.x & 63;
  const long long wv = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wv >= (long long)ntile * nslice) return false;
  const int slice = (int)(wv % nslice);
  const long long tile = t0 + wv / nslice;
  const int nlev = j.nlev;
  const int e0 = slice * 64 + lane;
  const bool act = e0 < j.chunk;
  const int e = act ? e0 : 0;   // (idle lanes of the last slice read element 0 and store nothing)
  const int s = e / nlev, kk = e - s * nlev;
  const bool in_main = e < j.main_e;
  cstep = in_main ? j.main_e : j.chunk - j.main_e;
  p = static_cast<const R2*>(j.prv) + (long long)b.tc * j.prv_tstride + tile * j.prv_tile_stride +
      (in_main ? e : (long long)j.ncol_p * j.main_e + (e - j.main_e)) + 3 * cstep;   // column 1 = slot 3
  const int nzm = b.sel.nz - 1;
  r.any = false;
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
    r.in[h] = ok;
    r.any = r.any || ok;
    r.o[h] = ok ? (sl - b.sel.sl0) + b.sel.n * (long long)k : 0;
  }
  return __ballot(r.any) != 0;   // (a slice none of whose elements is in the block, or owned: nothing to load)
}

// Plan layout, REGISTERS: a wave per (tile of the block, 64-element slice of the chunk).  R2: one 8-byte element (double,
// or the float2 of two adjacent slots); NBC: the bin class.
template <typename R2, int NBC>
__global__ void __launch_bounds__(256) wm_level_hist_kernel(const MpdataLevelHistJob b, const long long t0, const int ntile, const int nslice) {
  typedef Elem<R2> E;
  typedef typename E::R R;
  const R2* p;
  long long cstep;
  Rows<E::N> r;
  if (!hist_rows<R2>(b, t0, ntile, nslice, p, cstep, r)) return;
  const int nx = b.j.ncol_p - 6, nb = b.nb;
  R e[NBC + 1];
#pragma unroll
  for (int j = 0; j <= NBC; ++j) {
    e[j] = (R)b.e[j];                  // rounded once
    asm volatile("" : "+v"(e[j]));     // a vector register each: 33 scalar pairs beside the job do not fit the scalar file
  }
  const long long nout = b.sel.n * (long long)(b.sel.nz - 1);   // one (n, nzm) array per bin and value tracer
  const int ntr = b.bsum ? b.ntr : 0;
  unsigned q[E::N][NBC];
  R s[E::N][NBC];
  bool counted = false;
  if (ntr == 0) {
    march_hist<R2, NBC, true, false, false>(p, 0, cstep, nx, e, q, s);
    counted = true;
  }
  for (int jt = 0; jt < ntr; ++jt) {
    const int t = b.first + jt;
    const long long doff = (long long)(t - b.tc) * b.j.prv_tstride;   // signed: t < tc walks back
    if (jt == 0 && b.cnt) {   // the first walk also counts
      if (t == b.tc) march_hist<R2, NBC, true, true, false>(p, 0, cstep, nx, e, q, s);
      else march_hist<R2, NBC, true, true, true>(p, doff, cstep, nx, e, q, s);
      counted = true;
    } else {
      if (t == b.tc) march_hist<R2, NBC, false, true, false>(p, 0, cstep, nx, e, q, s);
      else march_hist<R2, NBC, false, true, true>(p, doff, cstep, nx, e, q, s);
    }
#pragma unroll
    for (int h = 0; h < E::N; ++h) {
      R* out = static_cast<R*>(b.bsum) + (r.o[h] + nout * ((long long)b.nb_all * jt));   // bin 0; a bin further: + nout
#pragma unroll
      for (int j = 0; j < NBC; ++j, out += nout) {
        asm volatile("" : "+v"(out));   // (kept a vector pointer: as scalar offsets the bins of a class spill the scalar file)
        if (j < nb) { if (r.in[h]) *out = s[h][j]; }   // (the outer test is wave-uniform)
      }
    }
  }
  if (counted && b.cnt) {
#pragma unroll
    for (int h = 0; h < E::N; ++h) {
      R* out = static_cast<R*>(b.cnt) + r.o[h];
#pragma unroll
      for (int j = 0; j < NBC; ++j, out += nout) {
        asm volatile("" : "+v"(out));
        if (j < nb) { if (r.in[h]) *out = (R)q[h][j]; }   // exact: nx < 2^24
      }
    }
  }
}

// Reference layout: element (sl, column i, level k, tracer t) at f + sl + ld * ((i + 2) + (nx + 6) * (k + nlev * t)); cnt at
// bi + n * (k + nlev * j), bsum at bi + n * (k + nlev * (j + nb * r)).  x: instances of the block, y: levels.
template <typename R, int NBC>
__global__ void __launch_bounds__(256) ref_level_hist_kernel(const R* f, const long long ld, const long long sl0, const long long n,
                                                            const int nx, const int nlev, const int tc, const int nb, const int nb_all, const Edges ed,
                                                            R* cnt, R* bsum, const int first, const int ntr) {
  const long long bi = (long long)blockIdx.x * 256 + threadIdx.x;
  if (bi >= n) return;
  const long long tstride = ld * ((long long)(nx + 6) * nlev);
  const long long nout = n * (long long)nlev;
  R e[NBC + 1];
#pragma unroll
  for (int j = 0; j <= NBC; ++j) {
    e[j] = (R)ed.e[j];
    asm volatile("" : "+v"(e[j]));   // (as in wm_level_hist_kernel)
  }
  for (long long k = blockIdx.y; k < nlev; k += gridDim.y) {
    const R* const p = f + (sl0 + bi) + ld * ((long long)(nx + 6) * (k + (long long)nlev * tc) + 3);   // column 1 of tracer tc
    const long long o = bi + n * k;
    unsigned q[1][NBC];
    R s[1][NBC];
    if (ntr == 0 || cnt) march_hist<R, NBC, true, false, false>(p, 0, ld, nx, e, q, s);
    if (cnt) {
#pragma unroll
      for (int j = 0; j < NBC; ++j)
        if (j < nb) cnt[o + nout * j] = (R)q[0][j];
    }
    for (int jt = 0; jt < ntr; ++jt) {
      const int t = first + jt;
      if (t == tc) march_hist<R, NBC, false, true, false>(p, 0, ld, nx, e, q, s);
      else march_hist<R, NBC, false, true, true>(p, tstride * (t - tc), ld, nx, e, q, s);   // signed
#pragma unroll
      for (int j = 0; j < NBC; ++j)
        if (j < nb) bsum[o + nout * (j + (long long)nb_all * jt)] = s[0][j];
    }
  }
}

bool bad_args(int ntr_all, int tc, int nb, const double* edges, const void* cnt, const void* bsum, int first, int ntr) {
  if (tc < 0 || tc >= ntr_all || nb < 1 || nb > MAXB || !edges || (!cnt && !bsum)) return true;
  for (int j = 0; j <= nb; ++j)
    if (edges[j] != edges[j] || (j < nb && edges[j] > edges[j + 1])) return true;
  return bsum && (first < 0 || ntr < 1 || first > ntr_all - ntr);
}

// e[0 .. nb] as given, +inf behind
void fill_edges(const double* edges, const int nb, double (&e)[MAXB + 1]) {
  for (int j = 0; j <= MAXB; ++j) e[j] = j <= nb ? edges[j] : std::numeric_limits<double>::infinity();
}

// the bins [g0, g0 + nbl) of a call of nb bins as a call of their own: its edges e[g0 .. g0 + nbl] (+inf behind), its outputs
// at bin g0 -- a column below e_g0 or above e_{g0 + nbl} is in no bin of the group
template <typename Ptr>
Ptr bin_at(Ptr a, const long long nout, const int g0, const int eb) {
  return a ? (Ptr)((char*)a + (size_t)nout * g0 * eb) : a;
}

}  // namespace

hipError_t mpdata_level_hist_wm(MpdataLevelHistJob& b, const double* edges, hipStream_t stream) {
  WmGrid g;
  if (bad_args(b.j.ntr, b.tc, b.nb, edges, b.cnt, b.bsum, b.first, b.ntr)) return hipErrorInvalidValue;
  const hipError_t e = wm_block_grid(b.j, b.sel, 1, &g);
  if (e != hipSuccess) return e;
  b.nb_all = b.nb;
  // bin groups: a walk carries at most GROUP bins (fp64 16, fp32 8: the largest classes whose resource report shows no
  // spill of either register file), a call of more bins is a walk per group; within a group the least bin class that holds it
  const int eb = b.sel.ipe == 1 ? 8 : 4, group = b.sel.ipe == 1 ? GROUP_F64 : GROUP_F32;
  const long long nout = b.sel.n * (long long)(b.sel.nz - 1);
  for (int g0 = 0; g0 < b.nb_all; g0 += group) {
    MpdataLevelHistJob c = b;
    c.nb = b.nb_all - g0 < group ? b.nb_all - g0 : group;
    fill_edges(edges + g0, c.nb, c.e);
    c.cnt = bin_at(b.cnt, nout, g0, eb);
    c.bsum = bin_at(b.bsum, nout, g0, eb);
    hipError_t el;
    if (b.sel.ipe == 1) {   // the class of 16 exists in fp64 alone
      void (*const k)(MpdataLevelHistJob, long long, int, int) = c.nb <= 4   ? wm_level_hist_kernel<double, 4>
                                                                 : c.nb <= 8 ? wm_level_hist_kernel<double, 8>
                                                                             : wm_level_hist_kernel<double, GROUP_F64>;
      el = wm_block_launch(k, k, c, g, stream);
    } else {
      void (*const k)(MpdataLevelHistJob, long long, int, int) =
          c.nb <= 4 ? wm_level_hist_kernel<float2, 4> : wm_level_hist_kernel<float2, GROUP_F32>;
      el = wm_block_launch(k, k, c, g, stream);
    }
    if (el != hipSuccess) return el;
  }
  return hipSuccess;
}

hipError_t mpdata_level_hist_ref(const void* f, int elem_bytes, long long ld, long long sl0, long long n, int nx, int nlev, int ntr_all,
                                 int tc, int nb, const double* edges, void* cnt, void* bsum, int first, int ntr, hipStream_t stream) {
  if (!f || ld < 1 || sl0 < 0 || n < 1 || sl0 + n > ld || nx < 1 || nlev < 1 || ntr_all < 1) return hipErrorInvalidValue;
  if (bad_args(ntr_all, tc, nb, edges, cnt, bsum, first, ntr)) return hipErrorInvalidValue;
  dim3 grid, block(256);
  if (ref_block_grid(n, nlev, &grid) != hipSuccess) return hipErrorInvalidValue;
  const long long nout = n * (long long)nlev;
  return ref_real(elem_bytes, [&](auto x) {
    typedef decltype(x) R;
    for (int g0 = 0; g0 < nb; g0 += 8) {   // groups of the one class
      Edges ed;
      const int nbl = nb - g0 < 8 ? nb - g0 : 8;
      fill_edges(edges + g0, nbl, ed.e);
      hipLaunchKernelGGL((ref_level_hist_kernel<R, 8>), grid, block, 0, stream, static_cast<const R*>(f), ld, sl0, n, nx, nlev, tc, nbl, nb,
                         ed, bin_at(static_cast<R*>(cnt), nout, g0, (int)sizeof(R)), bin_at(static_cast<R*>(bsum), nout, g0, (int)sizeof(R)),
                         first, bsum ? ntr : 0);
      const hipError_t el = hipGetLastError();
      if (el != hipSuccess) return el;
    }
    return hipSuccess;
  });
}
