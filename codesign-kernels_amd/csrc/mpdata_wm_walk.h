// mpdata_wm_walk.h -- what the calls on a block of instances of a resident plan share (include/mpdata_hip.h 3g .. 3r:
// the twelve kernel files mpdata_stats.hip, mpdata_courant.hip, mpdata_level_add.hip, mpdata_scale_uw.hip,
// mpdata_column_path.hip, mpdata_diffuse.hip, mpdata_subside.hip, mpdata_sediment.hip, mpdata_vsolve.hip, mpdata_cell_add.hip,
// mpdata_column_step.hip, mpdata_relax.hip; their host side is mpdata_plan_blocks.hip): the selector
// of the block, the element traits and the launch geometry.  Each of those files keeps its kernel whole -- the map wave -> (tracer, tile,
// element of the column chunk), the map slot -> (instance, tall level) and its march: moving the two maps into functions
// of this header changes the instructions of the plan-layout kernels (docs/EXPERIMENTS.md N), so they stay where
// they are until that form has been timed.
//   A wave owns 64 elements of a tile's column chunk ([tile][column][instance][level], the whole 128-byte lines of every
//   column first, the rests behind them: mpdata_layout.h) and walks the column slots as linear streams, NB columns in
//   flight.  The walk knows the storage layout only: LPS 8 .. 64, the one-instance-per-tile forms above 64 levels
//   (several 64-element slices per tile) and the windows of tall plans are the same code with other constants.
#ifndef MPDATA_WM_WALK_H
#define MPDATA_WM_WALK_H
#include <hip/hip_runtime.h>

#include "mpdata_layout.h"
#include "mpdata_windows.h"

// The block and the plan it is taken from.
//   sl0, n, ncrms: the block and the plan's size in REAL instances.  Slots that are no instance of the block -- the
//     padding of the last tile, the phantom half of an odd fp32 plan, the partner of a pair the block's ends split, a
//     neighbour in the tile -- reach no output and keep their bits (the one exception: the phantom follows the last slot in the calls that
//     rewrite the plan, mpdata_level_add.h, mpdata_scale_uw.h, mpdata_relax.h).
//   ipe: reals per 8-byte element -- 1 (fp64), 2 (fp32 plans: pairs of adjacent instances)
//   W = 1: the layout job describes the plan itself, nz = j.nlev + 1.
//   W > 1: the layout job describes the INNER plan of a windowed plan (mpdata_windows.h): slot q = sl * W + h is window
//     h of instance sl, nz the levels of the tall column.
struct MpdataBlockSel {
  long long sl0, n, ncrms;
  int ipe;
  int W, nz;
};

// everything below is for the twelve kernel files (`using namespace wm_walk`); a host file that builds the jobs needs the
// selector alone
namespace wm_walk {

constexpr int NB = 8;   // columns in flight per lane

// R2: one stored element -- 8 bytes of the plan layout (double, or the float2 of two adjacent instances), one real of
// the reference layout.  N reals R, half h by value (get) or in place (at).
template <typename R2> struct Elem;
template <> struct Elem<double> {
  typedef double R;
  static constexpr int N = 1;
  __device__ static double get(const double& v, int) { return v; }
  __device__ static double& at(double& v, int) { return v; }
};
template <> struct Elem<float2> {
  typedef float R;
  static constexpr int N = 2;
  __device__ static float get(const float2& v, int h) { return h ? v.y : v.x; }
  __device__ static float& at(float2& v, int h) { return h ? v.y : v.x; }
};
template <> struct Elem<float> {
  typedef float R;
  static constexpr int N = 1;
  __device__ static float get(const float& v, int) { return v; }
  __device__ static float& at(float& v, int) { return v; }
};

// ---- launch geometry: the grid covers the tiles the block touches (the phantom shares its 8-byte element, hence its
// tile, with the last slot).  j: a plan side exactly as wm_job makes it (strides in 8-byte elements; j.ref is not used);
// ntr: the tracers the grid runs over (1: a job without tracers).
struct WmGrid {
  long long t0;
  int ntile, nslice;
  unsigned blocks;   // of 256 threads
};
inline hipError_t wm_block_grid(const MpdataLayoutJob& j, const MpdataBlockSel& b, const int ntr, WmGrid* g) {
  if (!j.prv || ntr < 1 || j.nlev < 1 || j.slp < 1 || j.ntiles < 1 || j.ncol_p < 7 || j.ncols < 1 || j.prv_col0 < 0 ||
      j.prv_col0 + j.ncols > j.ncol_p || j.chunk != (long long)j.slp * j.nlev || j.main_e < 0 || j.main_e > j.chunk ||
      j.prv_tile_stride < (long long)j.ncol_p * j.chunk || (b.ipe != 1 && b.ipe != 2) || b.W < 1)
    return hipErrorInvalidValue;
  if (b.sl0 < 0 || b.n < 1 || b.sl0 + b.n > b.ncrms) return hipErrorInvalidValue;
  const long long spt = (long long)j.slp * b.ipe;   // slots per tile
  if (b.ncrms * b.W > (long long)j.ntiles * spt) return hipErrorInvalidValue;
  if (b.W == 1 ? b.nz != j.nlev + 1 : (j.slp != 1 || b.nz <= j.nlev + 1)) return hipErrorInvalidValue;
  const long long t0 = b.sl0 * b.W / spt, t1 = ((b.sl0 + b.n) * b.W - 1) / spt;
  const int nslice = (int)((j.chunk + 63) / 64);
  const long long waves = (long long)ntr * (t1 - t0 + 1) * nslice;
  if (t1 >= j.ntiles || t1 - t0 + 1 > 2147483647LL || (waves + 3) / 4 > 2147483647LL) return hipErrorInvalidValue;
  g->t0 = t0; g->ntile = (int)(t1 - t0 + 1); g->nslice = nslice; g->blocks = (unsigned)((waves + 3) / 4);
  return hipSuccess;
}
// the launch: kd for fp64 plans, kf for fp32 ones (float2 elements)
template <typename Job>
inline hipError_t wm_block_launch(void (*kd)(Job, long long, int, int), void (*kf)(Job, long long, int, int), const Job& b,
                                  const WmGrid& g, hipStream_t stream) {
  hipLaunchKernelGGL(b.sel.ipe == 1 ? kd : kf, dim3(g.blocks), dim3(256), 0, stream, b, g.t0, g.ntile, g.nslice);
  return hipGetLastError();
}

// reference layout: one thread per instance of the block (x, blocks of 256), y strides over the rows
inline hipError_t ref_block_grid(const long long n, const long long rows, dim3* grid) {
  const long long gx = (n + 255) / 256;
  if (gx > 2147483647LL) return hipErrorInvalidValue;
  *grid = dim3((unsigned)gx, (unsigned)(rows < 65535 ? rows : 65535));
  return hipSuccess;
}

}  // namespace wm_walk

#endif
