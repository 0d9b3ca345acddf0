// mpdata_column_scan.h -- host interface of the running column integral of one tracer of f into another, in place
// (mpdata_column_scan.hip; include/mpdata_hip.h 3aa): per instance sl of the block (b = sl - sl0) and INTERIOR column
// i = 1 .. nx, every statement one rounded operation in the arrays' precision, nothing contracted, every f the value
// before the call:
//   p(k) = wgt(b,k) * f(i,k,src)
//   UP:    s = +0;  k = 1 .. nlev            DOWN:  s = +0;  k = nlev .. 1
//     inclusive:  s = s + p(k);  o(k) = s    EXCLUSIVE:  o(k) = s;  s = s + p(k)
//   f(i,k,dst) = o(k);   total(b,i) = the final s
// wgt (n, nlev), total (n, nx): reference layout, leading dimension n, the block's first instance at index 0.  wgt NULL:
// rho(sl,k) * adz(sl,k), one rounded multiply, of the plan (a window: its own rho and adz).  total NULL: skipped.  Halo
// columns of f are neither read nor written; with dst != src the source tracer is only read.
#ifndef MPDATA_COLUMN_SCAN_H
#define MPDATA_COLUMN_SCAN_H
#include <hip/hip_runtime.h>

#include "mpdata_wm_walk.h"

#define MPDATA_COLUMN_SCAN_MODE_DOWN 1        // MPDATA_COLUMN_SCAN_DOWN of include/mpdata_hip.h
#define MPDATA_COLUMN_SCAN_MODE_EXCLUSIVE 2   // MPDATA_COLUMN_SCAN_EXCLUSIVE

// Plan layout.  j: the plan side of f exactly as wm_job(which = 0) makes it for the ONE tracer src (j.prv on it, j.ntr = 1,
// strides in 8-byte elements; j.ref is not used); dst lies at the signed offset doff = (dst - src) * j.prv_tstride from it.
// rho, adz, kc_tile_stride: as mpdata_column_path.h takes them (read only where wgt is NULL).
//   The geometry of mpdata_vsolve.hip: a workgroup takes UG adjacent units and CB columns, stages the column slots of src
//   and the weight row through LDS, a lane per (unit, column) sweeps its column in LDS in place and stores total, the waves
//   store LDS to the slots of dst.  down and excl are uniform per launch: one copy of the staging code.
//   sel: the block (mpdata_wm_walk.h).  A slot of dst that is no instance of the block keeps its bits: where an fp32
//     element holds a half the call does not write (the partner of a split pair, the phantom, in a window a level the
//     half does not own) that half is staged from DST, so it is stored back as loaded.  The PHANTOM of an odd fp32 plan
//     takes the result of the plan's last slot whenever the block holds that instance.
//     W > 1 (windowed plans): only the levels a window OWNS are read and written, each with the weight of the tall level
//     it stands for.  UP walks the windows upward, DOWN downward, s carried in the lane's registers: f is read once and
//     written once.  The phantom keeps its bits: the caller restores it.
struct MpdataColumnScanJob {
  MpdataLayoutJob j;
  MpdataBlockSel sel;
  long long doff;
  const void* wgt;            // NULL: rho * adz
  const void *rho, *adz;
  long long kc_tile_stride;
  void* total;                // NULL: not wanted
  int mode;
};
hipError_t mpdata_column_scan_wm(const MpdataColumnScanJob& b, hipStream_t stream);

// Reference layout: f(ld, -2:nx+3, nlev, ntr) with elem_bytes = 4 or 8, instances [sl0, sl0 + n) of its ld.  One thread per
// instance, grid.y over the columns, 64-bit offsets.  A thread owns its column of src and of dst and has read a level
// before it stores it.  wgt (n, nlev), or NULL with rho and adz (ld, nlev) of the plan.
hipError_t mpdata_column_scan_ref(void* f, int elem_bytes, long long ld, long long sl0, long long n, int nx, int nlev, int ntr, int src,
                                  int dst, const void* wgt, const void* rho, const void* adz, void* total, int mode, hipStream_t stream);

#endif
