// mpdata_layout.h -- host interface of the layout-conversion kernels (mpdata_layout.hip).
#ifndef MPDATA_LAYOUT_H
#define MPDATA_LAYOUT_H
#include <hip/hip_runtime.h>

// One array (all tracers of it) between the two layouts.
//   reference side: element (sl, column cs, level kk) of tracer tr at
//       ref + tr*ref_tstride + sl + ncrms*(cs*ref_colmul + kk*ref_levmul)
//     f, u, w: ref_colmul = 1, ref_levmul = number of columns; rho, rhow, adz, flux: one
//     column, ref_levmul = 1
//   private side: element e = s*nlev + kk (instance-in-tile s, level kk) of column
//   c = cs + prv_col0 of tile t at prv + tr*prv_tstride + t*prv_tile_stride +
//       c*chunk + e                                              (main_e == 0: unsplit arrays)
//       c*main_e + e                    if e <  main_e           (f, u, w: the whole 128-byte
//       ncol_p*main_e + c*rem_e + e - main_e   otherwise          lines of a column first)
struct MpdataLayoutJob {
  void* ref;
  void* prv;
  long long ncrms;
  int ncols;                 // columns of the reference-side array that are converted
  int nlev;                  // levels converted (nzm)
  int ntr;
  long long ref_colmul, ref_levmul, ref_tstride;
  int slp;                   // instances per tile
  int ntiles;
  int prv_col0;              // column shift: u, w start at c = 1 of the private column index
  long long chunk;           // slp * nlev
  long long main_e;          // elements of the line-aligned part of a column chunk (0: array not split)
  int ncol_p;                // column slots of a tile on the private side (split arrays)
  long long prv_tile_stride, prv_tstride;
};

hipError_t mpdata_layout_convert(const MpdataLayoutJob& j, int elem_bytes, bool to_private, hipStream_t stream);

// the split arrays (f, u, w: main_e > 0) column-walking: one workgroup per 64 (32) instances and array,
// all columns; nj = 1, or 2 arrays of equal nlev in one launch (u and w of an import)
hipError_t mpdata_layout_convert_cols(const MpdataLayoutJob* jobs, int nj, bool to_private, hipStream_t stream);

// import (reference -> plan) of f, u, w by 128-byte row segments through LDS-DMA; hipErrorNotSupported: conditions not
// met (odd ncrms, unaligned base, array of 4 GiB or more), take mpdata_layout_convert_cols
hipError_t mpdata_layout_import_rows(const MpdataLayoutJob* jobs, int nj, hipStream_t stream);

// fp32 plans with an odd ncrms (include/mpdata_hip.h 3f; (ncrms + 1) / 2 pairs, the upper half of the last one a phantom):
// whole arrays in single reals.  The jobs are the plan side as above (8-byte elements: pairs) but j.ncrms and
// j.ref_tstride count REALS of the reference side (leading dimension ncrms, odd).  Import fills the phantom and the
// padding pairs of the last tile with copies of instance ncrms - 1; no access leaves the caller's ncrms * rows reals.
// Any array (split or not); nj = 1, or 2 arrays of one plan in one launch.
hipError_t mpdata_layout_convert_odd(const MpdataLayoutJob* jobs, int nj, bool to_private, hipStream_t stream);
// the same invariant restored on the private side alone, after an import that moved single reals (blocks, windows):
// every slot (real) behind slot `last` := slot `last`, in the columns and tracers of the job
hipError_t mpdata_layout_refresh_phantom(const MpdataLayoutJob& j, long long last, hipStream_t stream);

// periodic lateral boundaries: f's halo columns -2..0, nx+1..nx+3 := copies of columns 1 + ((i-1) mod nx).
//   _wm: the plan layout, a job of f (wm_job(which = 0): ntr tracers, ncol_p = nx + 6), one wave per (tracer, tile);
//   _ref: a reference-layout array of ncols columns (column i at slot i + coff) and nlev levels per tracer, halo
//   columns ilo..0 and nx+1..ihi (f: ncols nx+6, coff 2, -2, nx+3; u: nx+5, 1, -1, nx+3; w: nx+4, 1, -1, nx+2)
hipError_t mpdata_layout_periodic_halo_wm(const MpdataLayoutJob& j, hipStream_t stream);
hipError_t mpdata_layout_periodic_halo_ref(void* a, int elem_bytes, long long ncrms, int nx, int ncols, int coff, int nlev,
                                           int ntr, int ilo, int ihi, hipStream_t stream);

// ---- blocks of instances (include/mpdata_hip.h 3d): instances [sl0, sl0 + n) of a plan <-> compact reference-layout
// arrays of leading dimension n.  A job of its own around the whole-plan one (the whole-plan kernels do not see it).
//   j: the plan side exactly as wm_job makes it for a whole-plan conversion (j.ncrms, j.ntiles, j.chunk, j.main_e,
//      the strides: in 8-byte elements of the private side); j.ref: the BLOCK's array, element (b, cs, kk) of tracer tr at
//      ref + tr*j.ref_tstride + b + n*(cs*ref_colmul + kk*ref_levmul), in reals (j.ref_tstride: for leading dimension n)
//   ipe: reals per 8-byte element of the private side -- 1 (fp64), 2 (fp32 plans: pairs of adjacent instances; a block
//      may split a pair, so both sides move single reals)
//   ncrms: the plan's instances (reals).  Import keeps the whole-plan invariant: the padding instances of the last tile
//      are copies of the plan's last instance (fp32: of its last pair) -- they follow a block that contains it.
struct MpdataBlockJob {
  MpdataLayoutJob j;
  long long sl0, n, ncrms;
  int ipe;
};
// one launch per array; the grid covers the tiles that intersect the block x the array's columns x tracers
hipError_t mpdata_layout_convert_block(const MpdataBlockJob& b, bool to_private, hipStream_t stream);
// rows x n elements between two pitched arrays (element (r, s) at base + r*pitch + s; pitches in elements of elem_bytes
// = 4 or 8): the slab a block is in a reference-layout array of leading dimension ncrms
hipError_t mpdata_layout_copy_rows(void* dst, const void* src, int elem_bytes, long long n, long long rows, long long dst_pitch,
                                   long long src_pitch, hipStream_t stream);

#endif
