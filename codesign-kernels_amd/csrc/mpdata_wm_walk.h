// mpdata_wm_walk.h -- what the calls on a block of instances of a resident plan share (include/mpdata_hip.h 3g .. 3ac:
// the twenty-three kernel files mpdata_stats.hip, mpdata_courant.hip, mpdata_level_add.hip, mpdata_scale_uw.hip,
// mpdata_column_path.hip, mpdata_diffuse.hip, mpdata_subside.hip, mpdata_sediment.hip, mpdata_vsolve.hip, mpdata_cell_add.hip,
// mpdata_column_step.hip, mpdata_relax.hip, mpdata_vdiffuse.hip, mpdata_convert.hip, mpdata_level_cov.hip, mpdata_level_cond.hip, mpdata_column_cond.hip, mpdata_nonneg.hip, mpdata_satadj.hip, mpdata_combine.hip, mpdata_column_scan.hip, mpdata_level_hist.hip, mpdata_level_draft.hip; their host side is mpdata_plan_blocks.hip): the selector of the block, the
// element traits, and on the host side the tile grid, the column-group geometry of the eight kernels that stage columns
// through LDS (col_groups_batched, col_groups_tiled), the LDS limit of a workgroup and the precision dispatch of the
// reference-layout launches (ref_real).  The host side is free to share: a launcher fills its kernel's argument struct
// from the result and the kernel is compiled as before.  Each of those files still keeps its kernel whole -- the map
// wave -> (tracer, tile, element of the column chunk), the map slot -> (instance, tall level) and its march: moving
// the two maps into functions of this header changes the instructions of the plan-layout kernels (docs/EXPERIMENTS.md
// N).  That form has been built and timed for the nine row kernels whose slot map is the same, relax .. level_draft
// (docs/EXPERIMENTS.md AN): no spelling keeps the occupancy of all their kernels, and the two benches run against the
// parent, level_hist and level_cond, miss the bar "the new side's best run does not exceed the parent's worst" in 7 of 40
// and 8 of 44 measurements, by up to 0.3 % and 1.5 %.  So the maps stay where they are.
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
//     rewrite the plan, mpdata_level_add.h, mpdata_scale_uw.h, mpdata_relax.h, mpdata_convert.h, mpdata_nonneg.h, mpdata_satadj.h, mpdata_combine.h, mpdata_column_scan.h).
//   ipe: reals per 8-byte element -- 1 (fp64), 2 (fp32 plans: pairs of adjacent instances)
//   W = 1: the layout job describes the plan itself, nz = j.nlev + 1.
//   W > 1: the layout job describes the INNER plan of a windowed plan (mpdata_windows.h): slot q = sl * W + h is window
//     h of instance sl, nz the levels of the tall column.
struct MpdataBlockSel {
  long long sl0, n, ncrms;
  int ipe;
  int W, nz;
};

// everything below is for the twenty-three kernel files (`using namespace wm_walk`); a host file that builds the jobs needs the
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
// ... and its precision: launch(R{}) with R = double or float by the bytes of a real (neither: refused), so that a
// launch is written once -- `typedef decltype(r) R;` inside the generic lambda names the type
template <typename F>
inline hipError_t ref_real(const int elem_bytes, F&& launch) {
  return elem_bytes == 8 ? launch(double{}) : elem_bytes == 4 ? launch(float{}) : hipErrorInvalidValue;
}

// ---- column groups: the workgroups of the kernels that stage whole columns of a group of instances through LDS
// (mpdata_column_path.hip, mpdata_vsolve.hip, mpdata_column_step.hip, mpdata_vdiffuse.hip, mpdata_column_cond.hip, mpdata_column_scan.hip: columns in batches; mpdata_sediment.hip,
// mpdata_cell_add.hip: CB columns in flight, a tile per wave).  A UNIT is one 8-byte element of the instance axis (an
// instance, or the pair 2 * ue, 2 * ue + 1 of an fp32 plan): slot ue % slp of tile ue / slp, or, in a windowed plan, the
// tiles ue * W .. ue * W + W - 1.  A workgroup takes UG adjacent units (a power of two, a multiple of slp) and CB
// adjacent columns, re-laid in LDS as [column][unit][ns] with an odd level stride ns.  16 units make a row of a
// per-instance array of the group whole 128-byte lines (32 where a tile holds 8: a tile per wave while staging); fewer
// where the LDS does not hold them.
constexpr int LDS_ELEMS = 5120;   // 8-byte elements of LDS per workgroup at most (40 KiB: room for four workgroups per CU)

struct ColGroups {
  int UG, ush;              // units of a group, UG = 1 << ush
  int CB, ncb;              // columns of a batch; batches (tiled: 1)
  int ns;                   // level stride in LDS (odd)
  int nround;               // tiled: tiles per wave
  long long g0, ngroup;     // first group, groups (both fit an int where the units do: UG >= slp)
  long long lds_e;          // 8-byte elements of LDS of the launch
};

// the result into the fields all eight argument structs have (g0, ngroup: int; long long in column_path's)
template <typename Args>
inline void col_groups_fill(const ColGroups& c, Args* a) {
  a->UG = c.UG; a->CB = c.CB; a->ns = c.ns;
  a->g0 = static_cast<decltype(a->g0)>(c.g0); a->ngroup = static_cast<decltype(a->ngroup)>(c.ngroup);
}

// what the two rules share, behind UG, CB, ncb and lds_e: the groups the block's tiles touch and the union of the
// launchers' guards.  unit_mul: what the kernel multiplies a unit by in int arithmetic -- 1, W where it forms tiles of a
// windowed plan from units (mpdata_vsolve.hip, mpdata_column_scan.hip), 0 where it counts units in long long (mpdata_column_path.hip, mpdata_column_cond.hip: their groups
// may lie beyond 2^31 units, and it goes on running such a plan).
//   UG is a power of two: it starts at 16 or 4 * slp and halves, and slp is 1, 2, 4 or 8 in every plan mpdata_plan_create
//     makes (64 / LPS; 1 above 64 levels and in the inner plan of a windowed one), so the test refuses no plan of the
//     one launcher that did not have it (column_path divides where the others shift).
//   lds_e <= budget follows from how both rules pick CB -- batched: CB + rows <= (budget - fixed) / (UG * ns); tiled:
//     bufs * CB * UG * ns <= budget - held -- wherever CB >= 1, which both have checked: the test cannot fire today and
//     stands guard over a rule that replaces one of them.
inline bool col_groups_range(const MpdataLayoutJob& j, const MpdataBlockSel& b, const WmGrid& wg, const int budget, const int unit_mul,
                             ColGroups* g) {
  g->ush = 0;
  while ((1 << g->ush) < g->UG) ++g->ush;   // (UG <= 256)
  if ((1 << g->ush) != g->UG) return false;
  const long long t1 = wg.t0 + wg.ntile - 1;
  const long long ue_first = wg.t0 / b.W * j.slp, ue_last = t1 / b.W * j.slp + j.slp - 1;
  g->g0 = ue_first / g->UG;
  g->ngroup = ue_last / g->UG - g->g0 + 1;
  // (blockIdx.x; unit and tile arithmetic of the kernels is in int)
  return g->ngroup <= 2147483647LL / ((long long)j.ntr * g->ncb) && (ue_last + g->UG) * unit_mul <= 2147483647LL && g->lds_e <= budget;
}

// Columns in batches over blockIdx.x: next to CB columns the LDS holds `rows` coefficient rows [unit][ns] and `fixed`
// elements (the window table, the array addresses); UG halves until one column and the rows fit, then the batches are
// made even.  budget: LDS_ELEMS, or less for more workgroups per CU.  j, b, wg: as wm_block_grid took and made them.
inline bool col_groups_batched(const MpdataLayoutJob& j, const MpdataBlockSel& b, const WmGrid& wg, const int budget, const int fixed,
                               const int rows, const int unit_mul, ColGroups* g) {
  const int nx = j.ncol_p - 6, slp = j.slp, room = budget - fixed;
  g->ns = j.nlev | 1;
  g->nround = 0;
  g->UG = slp >= 8 ? 4 * slp : 16;
  while (g->UG > slp && (long long)g->UG * g->ns * (1 + rows) > room) g->UG /= 2;
  if (g->UG % slp || (long long)g->UG * g->ns * (1 + rows) > room || g->UG > 256) return false;
  int cbmax = (int)(room / ((long long)g->UG * g->ns)) - rows;
  if (cbmax > 256 / g->UG) cbmax = 256 / g->UG;   // (a lane per (column, unit) pair)
  if (cbmax > nx) cbmax = nx;
  g->ncb = (nx + cbmax - 1) / cbmax;
  g->CB = (nx + g->ncb - 1) / g->ncb;   // even batches
  g->lds_e = (long long)(g->CB + rows) * g->UG * g->ns + fixed;
  return col_groups_range(j, b, wg, budget, unit_mul, g);
}

// A tile per wave, all columns in one workgroup, the windows over blockIdx.y: the LDS holds `bufs` buffers of CB <= NB
// columns in flight, `rows` coefficient rows, with `sums` the running sums of nround tiles per wave (256 elements a
// round) and `fixed` elements; UG halves until two columns fit.  wide: 32 units where a tile holds 8.  What the callers
// say of their guards holds here: a tile is a workgroup's at most (nslice <= 4: 256 elements of a chunk), W <= 65535 is
// gridDim.y, a lane per instance of the group; none is reached by a plan mpdata_plan_create makes, and a new tiling that
// breaks one must extend the kernels and fails here, before any launch, until it does.
inline bool col_groups_tiled(const MpdataLayoutJob& j, const MpdataBlockSel& b, const WmGrid& wg, const int budget, const int fixed,
                             const int rows, const int bufs, const bool sums, const bool wide, ColGroups* g) {
  if (wg.nslice > 4 || b.W > 65535) return false;
  const int nx = j.ncol_p - 6, slp = j.slp, tpw = 4 / wg.nslice;
  g->ns = j.nlev | 1;
  g->ncb = 1;
  g->UG = wide && slp >= 8 ? 4 * slp : slp > 16 ? slp : 16;
  for (;;) {
    const long long per_col = (long long)g->UG * g->ns;
    g->nround = (g->UG / slp + tpw - 1) / tpw;
    const long long held = fixed + rows * per_col + (sums ? (long long)g->nround * 256 : 0);
    long long cb = (budget - held) / (bufs * per_col);
    if (cb < 0) cb = 0;
    if (cb > NB) cb = NB;
    if (cb > nx) cb = nx;
    g->CB = (int)cb;
    g->lds_e = bufs * cb * per_col + held;
    if (g->CB >= 2 || g->CB >= nx || g->UG <= slp) break;
    g->UG /= 2;
  }
  if (g->CB < 1 || g->UG % slp || (long long)g->UG * b.ipe > 256) return false;
  return col_groups_range(j, b, wg, budget, 1, g);
}

}  // namespace wm_walk

#endif
