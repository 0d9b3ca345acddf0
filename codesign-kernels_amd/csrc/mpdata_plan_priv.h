// mpdata_plan_priv.h -- what the two translation units of the plan API share: the plan itself and the helpers both use.
//   mpdata_plan.hip         create, import / export (whole and blocks, 3d), run, multi-GPU handles, destroy
//   mpdata_plan_blocks.hip  the calls on a block of instances of a resident plan (include/mpdata_hip.h 3g .. 3m)
#ifndef MPDATA_PLAN_PRIV_H
#define MPDATA_PLAN_PRIV_H
#include "mpdata_internal.h"

struct mpdata_plan {
  int64_t ncrms;
  int nx, nz, ntracers;
  int eb;        // bytes per real: 8 (fp64 plan) or 4 (fp32 plan)
  int device;    // the plan's device
  int variant;   // MPDATA_VARIANT_* at creation
  int layout;    // MPDATA_LAYOUT_*
  mpd::Sizes sz; // element counts of the reference-layout arrays
  // reference-layout plans
  mpd::Arena arena;
  void *f, *u, *w, *rho, *rhow, *adz, *flux;  // = arena.p[0..6]
  // wave-major plans
  int lps, slp, wpb, ntiles;
  int64_t wm_ncrms;  // instances as the wave-major side sees them: ncrms (fp64) or (ncrms + 1) / 2 pairs (fp32)
  // fp32 plans with an odd ncrms (include/mpdata_hip.h 3f): the upper half of the last pair is a phantom.  INVARIANT: in
  // every plan array it is a copy of instance ncrms - 1, and the padding pairs of the last tile are copies of that pair.
  // Whole imports keep it themselves (mpdata_layout_convert_odd); plan_phantom restores it behind everything else that
  // replaces instance ncrms - 1.  No export reads it.
  bool odd;
  long long chunk, tile_elems, main_e;   // main_e: elements of the line-aligned part of a column chunk
  void *pf, *pu, *pw, *pkc, *pflux;  // private arrays
  void* stage;                       // reference-layout staging: one tracer of f (or u, w)
  size_t stage_elems;
  void* bstage;                      // block staging: what the host forms of the block calls (3d download, 3g .. 3m) put on
  size_t bstage_bytes;               // the device, packed in argument order (plan_bstage; grown on demand)
  void* dbuf;                        // scratch of the calls that rewrite f from its old values (plan_dbuf; grown on demand):
  size_t dbuf_bytes;                 // 3l tkh in the plan layout (wave-major) or the new interior (reference layout), 3m the new rows
  void* flux_ref;                    // flux in the reference layout (level nz is carried through)
  void* wpark;                       // EXACT: park array of the limited vertical fluxes (bit-identical flux); with park_regs
  size_t wpark_bytes;                // only mpdata_plan_run_uw needs it: allocated by its first call
  bool park_regs;                    // EXACT, nx <= MPDATA_WM_NPK: mpdata_plan_run parks in registers (no park array)
  hipStream_t stream;
  bool own_stream;
  hipEvent_t ev0, ev1;
  bool uploaded, ran;
  bool have_u, have_w;   // the plan holds velocities (imported since the last mpdata_plan_run_uw)
  bool timing;     // record the event pair around every run (mpdata_plan_last_kernel_ms); mpdata_plan_set_timing
  unsigned runs;   // launches so far (serpentine tile order)
  int boundary;    // MPDATA_BOUNDARY_* (mpdata_plan_set_boundary)
  // per tracer: f's halo columns hold copies of its interior (set by the halo kernel; cleared by an import of f and
  // by every run, whose kernels leave first-pass values there)
  unsigned char* halo_ok;
  // windowed plans (include/mpdata_hip.h 3e; nz > 238): `inner` is an ordinary wave-major plan whose ncrms * W instances
  // are the W level windows (mpdata_windows.h) of this plan's instances, window index fastest.  It runs on this plan's
  // stream with this plan's boundary mode and shares halo_ok; of the fields above this plan itself uses the sizes,
  // stage (tall reference-layout staging of host transfers), bstage, flux_ref (level nz), the stream, the events
  // and the state flags.
  mpdata_plan* inner;
  int W;
  // per tracer: every non-owned level of every window of f holds its owner's value (set by a whole import of f and by
  // the seam refresh; cleared by every run, which leaves the 3 + 3 margin levels of a seam wrong)
  unsigned char* seam_ok;
  mpdata_multi* multi;  // != null: a multi-GPU plan (mpdata_multi.hip); nothing else above is used
};

#pragma GCC visibility push(hidden)
namespace mpd {
// layout jobs of a wave-major plan (which = 0 f, 1 u, 2 w, 3 rho, 4 rhow, 5 adz, 6 flux), whole and of a block
MpdataLayoutJob wm_job(const mpdata_plan* p, int which, void* ref, int first_tracer, int ntr);
MpdataBlockJob wm_block_job(const mpdata_plan* p, int which, void* ref, int64_t sl0, int64_t n, int first_tracer, int ntr);
// argument checks (set the error text): the plan's precision, a tracer range, a block of instances
int plan_check(const mpdata_plan* p, int eb);
int tracer_range(const mpdata_plan* p, int first, int count);
int block_range(const char* what, const mpdata_plan* p, int64_t sl0, int64_t n);
int plan_bstage(mpdata_plan* p, size_t need);             // the block staging buffer, at least `need` bytes
int plan_wrap_f(mpdata_plan* p, int first, int count);    // periodic plans: wrap the stale halos of f
int plan_seams(mpdata_plan* p, int first, int count);     // windowed plans: refresh the stale seams of f
int plan_phantom(mpdata_plan* p, int which, int first, int ntr);   // odd fp32 plans: the phantom follows the last instance
bool legacy_convert();                                    // MPDATA_LAYOUT_LEGACY=1 (A/B)
}  // namespace mpd
#pragma GCC visibility pop

#endif
