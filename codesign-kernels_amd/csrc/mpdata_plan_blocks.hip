// mpdata_plan_blocks.hip -- the calls on a block of instances of a resident plan (include/mpdata_hip.h 3g .. 3ac).  Host
// code only: the kernels are in mpdata_stats.hip .. mpdata_level_draft.hip.  A call is its kernel file, a dispatch on the
// layout (plan_X), one check function for both of its forms (plan_X_check) and, for the host form, a table of its arrays;
// the tails the calls share are array_block, scratch_done and plan_rewrote.
#include <cstring>

#include "mpdata_cell_add.h"
#include "mpdata_column_path.h"
#include "mpdata_column_scan.h"
#include "mpdata_column_step.h"
#include "mpdata_combine.h"
#include "mpdata_convert.h"
#include "mpdata_courant.h"
#include "mpdata_diffuse.h"
#include "mpdata_level_add.h"
#include "mpdata_level_cond.h"
#include "mpdata_column_cond.h"
#include "mpdata_level_cov.h"
#include "mpdata_level_draft.h"
#include "mpdata_level_hist.h"
#include "mpdata_nonneg.h"
#include "mpdata_plan_priv.h"
#include "mpdata_relax.h"
#include "mpdata_satadj.h"
#include "mpdata_scale_uw.h"
#include "mpdata_sediment.h"
#include "mpdata_stats.h"
#include "mpdata_subside.h"
#include "mpdata_vdiffuse.h"
#include "mpdata_vsolve.h"

using namespace mpd;

namespace {

// the plan's scratch buffer (struct mpdata_plan: dbuf), grown as the block staging buffer is
int plan_dbuf(mpdata_plan* p, size_t need) {
  if (p->dbuf_bytes >= need) return 0;
  HIP_TRY(hipStreamSynchronize(p->stream));
  if (p->dbuf) (void)hipFree(p->dbuf);
  p->dbuf = nullptr; p->dbuf_bytes = 0;
  HIP_TRY(hipMalloc(&p->dbuf, need));
  p->dbuf_bytes = need;
  return 0;
}
// a block of a plan for the kernels that walk its plan layout (mpdata_wm_walk.h), with wm_plan(p) the plan the layout
// jobs are made of: a windowed plan's inner plan, read and rewritten where it lies (its stream and boundary are not
// forwarded: nothing of it runs)
MpdataBlockSel block_sel(const mpdata_plan* p, int64_t sl0, int64_t n) {
  MpdataBlockSel b;
  b.sl0 = sl0; b.n = n; b.ncrms = p->ncrms; b.ipe = 8 / p->eb;
  b.W = p->inner ? p->W : 1; b.nz = p->nz;
  return b;
}
const mpdata_plan* wm_plan(const mpdata_plan* p) { return p->inner ? p->inner : p; }
// the plan is walked in its plan layout (else: a reference-layout plan, whose arrays the *_ref kernels take)
bool plan_walked(const mpdata_plan* p) { return p->inner || p->layout == MPDATA_LAYOUT_WAVEMAJOR; }
// tracer `first` of a reference-layout plan's f
char* ref_f(const mpdata_plan* p, int first) { return (char*)p->f + (size_t)first * (p->sz.f / p->ntracers) * p->eb; }
// rho and adz of a wave-major plan's kc array ([tile][rho, adz, rhow][chunk]) into the three fields of a job
template <typename Job>
void kc_rho_adz(const mpdata_plan* q, Job& b) {
  const MpdataLayoutJob jr = wm_job(q, 3, nullptr, 0, 1), ja = wm_job(q, 5, nullptr, 0, 1);
  b.rho = (const double*)jr.prv + jr.prv_col0 * jr.chunk;
  b.adz = (const double*)ja.prv + ja.prv_col0 * ja.chunk;
  b.kc_tile_stride = jr.prv_tile_stride;
}

// ---- Argument checks.  Every plan_X_check(what, ..., eb) serves both forms of its call (eb = 0: the device form) and
// checks in one order: block_ranges (block_range alone for a call without tracers), the call's own arguments, plan_state.
// A host form takes all tracers: it has no range to check and passes none.
int block_ranges(const char* what, const mpdata_plan* p, int64_t sl0, int64_t n, int first, int count, int eb) {
  const int rc = block_range(what, p, sl0, n);
  return rc || eb ? rc : tracer_range(p, first, count);
}
// the state a call on the plan's velocities needs: filled once, and the arrays asked for still held
int plan_uw_state(const char* what, const mpdata_plan* p, bool need_u, bool need_w) {
  if (!p->uploaded) return set_err(MPDATA_ESTATE, "%s before upload / import", what);
  if ((need_u && !p->have_u) || (need_w && !p->have_w))
    return set_err(MPDATA_ESTATE, "%s: the plan does not hold %s (mpdata_plan_run_uw used them up: import u and w)", what,
                   (need_u && !p->have_u) ? "u" : "w");
  return 0;
}
// what the plan is (host forms: its precision) and holds
int plan_state(const char* what, const mpdata_plan* p, int eb, bool need_u = false, bool need_w = false) {
  const int rc = eb ? plan_check(p, eb) : 0;
  return rc ? rc : plan_uw_state(what, p, need_u, need_w);
}
int cell_add_mode(const char* what, int mode) {
  if (mode != MPDATA_CELL_ADD && mode != MPDATA_CELL_ADD_CLIP) return set_err(MPDATA_EINVAL, "%s: unknown mode %d", what, mode);
  return 0;
}
int level_add_mode(const char* what, int mode) {
  if (mode != MPDATA_LEVEL_ADD && mode != MPDATA_LEVEL_ADD_CLIP) return set_err(MPDATA_EINVAL, "%s: unknown mode %d", what, mode);
  return 0;
}
// the sizes of a call on reference-layout device arrays (ntracers = NULL: a call without tracers)
int array_sizes(const char* what, int64_t ncrms, int nx, int nz, const int* ntracers) {
  if (ncrms >= 1 && nx >= 1 && nz >= 2 && (!ntracers || *ntracers >= 1)) return 0;
  if (!ntracers) return set_err(MPDATA_EINVAL, "%s: bad sizes ncrms=%lld nx=%d nz=%d (need >=1,>=1,>=2)", what, (long long)ncrms, nx, nz);
  return set_err(MPDATA_EINVAL, "%s: bad sizes ncrms=%lld nx=%d nz=%d ntracers=%d (need >=1,>=1,>=2,>=1)", what, (long long)ncrms, nx,
                 nz, *ntracers);
}
// the instance range of an array form that takes a block
int array_block(const char* what, int64_t ncrms, int64_t sl0, int64_t n) {
  if (n >= 1 && sl0 >= 0 && sl0 <= ncrms - n) return 0;
  return set_err(MPDATA_EINVAL, "%s: instances [%lld, %lld) outside the arrays' %lld", what, (long long)sl0, (long long)(sl0 + n),
                 (long long)ncrms);
}
// the end of an array form whose work (e: what issuing it returned) goes through a scratch array of the call's own: the
// array is freed when the work is done, so the call returns after it
int scratch_done(void* scratch, void* stream, hipError_t e) {
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  (void)hipFree(scratch);
  HIP_TRY(e);
  return 0;
}
// the marks of the tracer range after a call has rewritten owned levels (SEAMS: the other copies of a windowed plan are
// stale, and the inner plan's phantom follows a block that ends the plan, as after a seam refresh) or interior columns
// (HALOS: a periodic plan's halos are copies of the old interior) of f of the block
enum { SEAMS = 1, HALOS = 2 };
int plan_rewrote(mpdata_plan* p, int64_t sl0, int64_t n, int first, int count, int marks) {
  if ((marks & SEAMS) && p->inner) {
    memset(p->seam_ok + first, 0, (size_t)count);
    const int rc = sl0 + n == p->ncrms ? plan_phantom(p->inner, 0, first, count) : 0;
    if (rc) return rc;
  }
  if ((marks & HALOS) && p->boundary == MPDATA_BOUNDARY_PERIODIC) memset(p->halo_ok + first, 0, (size_t)count);
  return 0;
}

// ---- Host forms (all tracers, synchronous): the host arrays of a call go through the plan's block staging buffer, in
// argument order without padding; an absent array takes no room and gets a NULL device address.  Element alignment is all
// the kernels need of these arrays -- they read them one real at a time -- but for tkh, which feeds the layout conversion
// of wave-major plans (its fast path looks at the alignment of the base): it is the first of its call, at offset 0.
struct HostArr {
  const void* host;   // NULL: absent
  size_t bytes;
  bool out;           // false: read by the call (H2D in front of it); true: written by it (D2H behind it)
  void* dev = nullptr;
};
// sizes the buffer, assigns the device addresses and issues the H2D copies on the plan's stream
template <int N>
int stage_in(mpdata_plan* p, HostArr (&a)[N]) {
  size_t need = 0, off = 0;
  for (const HostArr& h : a) need += h.host ? h.bytes : 0;
  const int rc = plan_bstage(p, need);
  if (rc) return rc;
  for (HostArr& h : a) {
    if (!h.host) continue;
    h.dev = (char*)p->bstage + off;
    off += h.bytes;
    if (!h.out) HIP_TRY(hipMemcpyAsync(h.dev, h.host, h.bytes, hipMemcpyHostToDevice, p->stream));
  }
  return 0;
}
// ... and behind the call the D2H copies and the synchronisation
template <int N>
int stage_out(mpdata_plan* p, const HostArr (&a)[N]) {
  for (const HostArr& h : a)
    if (h.host && h.out) HIP_TRY(hipMemcpyAsync(const_cast<void*>(h.host), h.dev, h.bytes, hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  return 0;
}

// 3y: the caller's numbers in the precision R, each rounded once, and the three derived ones, each operation rounded once
template <typename R>
void satadj_par(const mpdata_satadj_params* s, MpdataSatadjPar<R>* o) {
  for (int c = 0; c < 9; ++c) {
    o->esw[c] = (R)s->esw[c]; o->desw[c] = (R)s->desw[c];
    o->esi[c] = (R)s->esi[c]; o->desi[c] = (R)s->desi[c];
  }
  o->t0 = (R)s->t0; o->xmin = (R)s->xmin; o->eps = (R)s->eps; o->lv = (R)s->lv; o->ls = (R)s->ls;
  o->tmin = (R)s->tmin; o->tmax = (R)s->tmax; o->tol = (R)s->tol; o->maxit = s->maxit;
  o->an = (R)1 / (o->tmax - o->tmin);
  o->bn = o->tmin * o->an;
  o->lf = o->ls - o->lv;
}

}  // namespace

extern "C" {

// ---- 3g: horizontal sum / min / max per level of f.  Reads f, writes the outputs: no flag of the plan is touched (the
// halo and seam marks stay -- halo columns are not read, owned levels are right whatever the seams hold), no event is
// recorded, and a windowed plan's inner plan is read where it lies (its stream and boundary are not forwarded: nothing
// of it runs).
static int plan_level_stats(mpdata_plan* p, int64_t sl0, int64_t n, void* sum, void* mn, void* mx, int first, int count) {
  if (plan_walked(p)) {
    MpdataStatsJob b;
    b.j = wm_job(wm_plan(p), 0, nullptr, first, count);
    b.sel = block_sel(p, sl0, n);
    b.sum = sum; b.mn = mn; b.mx = mx;
    HIP_TRY(mpdata_stats_wm(b, p->stream));
  } else {
    HIP_TRY(mpdata_stats_ref(ref_f(p, first), p->eb, p->ncrms, sl0, n, p->nx, p->nz - 1, count, sum, mn, mx, p->stream));
  }
  return 0;
}
static int plan_level_stats_check(const char* what, const mpdata_plan* p, int64_t sl0, int64_t n, const void* sum, const void* mn,
                                  const void* mx, int first, int count, int eb) {
  const int rc = block_ranges(what, p, sl0, n, first, count, eb);
  if (rc) return rc;
  if (!sum && !mn && !mx) return set_err(MPDATA_EINVAL, "%s: sum, min and max are all NULL", what);
  return plan_state(what, p, eb);
}
int mpdata_plan_level_stats_device(mpdata_plan* p, int64_t sl0, int64_t n, void* sum, void* mn, void* mx, int first_tracer,
                                   int ntracers) {
  const int rc = plan_level_stats_check("mpdata_plan_level_stats_device", p, sl0, n, sum, mn, mx, first_tracer, ntracers, 0);
  if (rc) return rc;
  DevGuard g(p->device);
  return plan_level_stats(p, sl0, n, sum, mn, mx, first_tracer, ntracers);
}
static int plan_level_stats_host(mpdata_plan* p, int64_t sl0, int64_t n, void* sum, void* mn, void* mx, int eb) {
  int rc = plan_level_stats_check("mpdata_plan_level_stats", p, sl0, n, sum, mn, mx, 0, 0, eb);
  if (rc) return rc;
  DevGuard g(p->device);
  const size_t one = (size_t)n * (p->nz - 1) * p->ntracers * eb;
  HostArr a[3] = {{sum, one, true}, {mn, one, true}, {mx, one, true}};
  rc = stage_in(p, a);
  if (!rc) rc = plan_level_stats(p, sl0, n, a[0].dev, a[1].dev, a[2].dev, 0, p->ntracers);
  return rc ? rc : stage_out(p, a);
}
int mpdata_plan_level_stats(mpdata_plan* p, int64_t sl0, int64_t n, double* sum, double* mn, double* mx) {
  return plan_level_stats_host(p, sl0, n, sum, mn, mx, 8);
}
int mpdata_plan_level_stats_f32(mpdata_plan* p, int64_t sl0, int64_t n, float* sum, float* mn, float* mx) {
  return plan_level_stats_host(p, sl0, n, sum, mn, mx, 4);
}
// the same reduction on a reference-layout device array (arguments checked before any device call)
static int level_stats_array(int64_t ncrms, int nx, int nz, int ntracers, const void* f, void* sum, void* mn, void* mx, void* stream,
                             int eb) {
  const int rc = array_sizes("mpdata_level_stats_device", ncrms, nx, nz, &ntracers);
  if (rc) return rc;
  if (!f) return set_err(MPDATA_EINVAL, "mpdata_level_stats_device: null f");
  if (!sum && !mn && !mx) return set_err(MPDATA_EINVAL, "mpdata_level_stats_device: sum, min and max are all NULL");
  HIP_TRY(mpdata_stats_ref(f, eb, ncrms, 0, ncrms, nx, nz - 1, ntracers, sum, mn, mx, (hipStream_t)stream));
  return 0;
}
int mpdata_level_stats_device(int64_t ncrms, int nx, int nz, int ntracers, const double* f, double* sum, double* mn, double* mx,
                              void* stream) {
  return level_stats_array(ncrms, nx, nz, ntracers, f, sum, mn, mx, stream, 8);
}
int mpdata_level_stats_f32_device(int64_t ncrms, int nx, int nz, int ntracers, const float* f, float* sum, float* mn, float* mx,
                                  void* stream) {
  return level_stats_array(ncrms, nx, nz, ntracers, f, sum, mn, mx, stream, 4);
}

// ---- 3h: outflow Courant number of the plan's velocities per level (clev) and per instance (cinst).  Reads u, w, rho,
// adz, writes the outputs: as the level statistics above no flag of the plan is touched, no event is recorded, and a
// windowed plan's inner plan is read where it lies.
static int plan_courant(mpdata_plan* p, int64_t sl0, int64_t n, void* clev, void* cinst) {
  if (plan_walked(p)) {
    const mpdata_plan* q = wm_plan(p);
    MpdataCourantJob b;
    b.j = wm_job(q, 1, nullptr, 0, 1);
    b.w = wm_job(q, 2, nullptr, 0, 1).prv;
    kc_rho_adz(q, b);
    b.sel = block_sel(p, sl0, n);
    b.clev = clev; b.cinst = cinst;
    HIP_TRY(mpdata_courant_wm(b, p->stream));
  } else {
    HIP_TRY(mpdata_courant_ref(p->u, p->w, p->rho, p->adz, p->eb, p->ncrms, sl0, n, p->nx, p->nz, clev, cinst, p->stream));
  }
  return 0;
}
static int plan_courant_check(const char* what, const mpdata_plan* p, int64_t sl0, int64_t n, const void* clev, const void* cinst,
                              int eb) {
  const int rc = block_range(what, p, sl0, n);
  if (rc) return rc;
  if (!clev && !cinst) return set_err(MPDATA_EINVAL, "%s: clev and cinst are both NULL", what);
  return plan_state(what, p, eb, true, true);
}
int mpdata_plan_courant_device(mpdata_plan* p, int64_t sl0, int64_t n, void* clev, void* cinst) {
  const int rc = plan_courant_check("mpdata_plan_courant_device", p, sl0, n, clev, cinst, 0);
  if (rc) return rc;
  DevGuard g(p->device);
  return plan_courant(p, sl0, n, clev, cinst);
}
static int plan_courant_host(mpdata_plan* p, int64_t sl0, int64_t n, void* clev, void* cinst, int eb) {
  int rc = plan_courant_check("mpdata_plan_courant", p, sl0, n, clev, cinst, eb);
  if (rc) return rc;
  DevGuard g(p->device);
  HostArr a[2] = {{clev, (size_t)n * (p->nz - 1) * eb, true}, {cinst, (size_t)n * eb, true}};
  rc = stage_in(p, a);
  if (!rc) rc = plan_courant(p, sl0, n, a[0].dev, a[1].dev);
  return rc ? rc : stage_out(p, a);
}
int mpdata_plan_courant(mpdata_plan* p, int64_t sl0, int64_t n, double* clev, double* cinst) {
  return plan_courant_host(p, sl0, n, clev, cinst, 8);
}
int mpdata_plan_courant_f32(mpdata_plan* p, int64_t sl0, int64_t n, float* clev, float* cinst) {
  return plan_courant_host(p, sl0, n, clev, cinst, 4);
}
// the same reduction on reference-layout device arrays (arguments checked before any device call)
static int courant_array(int64_t ncrms, int nx, int nz, const void* u, const void* w, const void* rho, const void* adz, void* clev,
                         void* cinst, void* stream, int eb) {
  const int rc = array_sizes("mpdata_courant_device", ncrms, nx, nz, nullptr);
  if (rc) return rc;
  if (!u || !w || !rho || !adz)
    return set_err(MPDATA_EINVAL, "mpdata_courant_device: null %s", !u ? "u" : !w ? "w" : !rho ? "rho" : "adz");
  if (!clev && !cinst) return set_err(MPDATA_EINVAL, "mpdata_courant_device: clev and cinst are both NULL");
  HIP_TRY(mpdata_courant_ref(u, w, rho, adz, eb, ncrms, 0, ncrms, nx, nz, clev, cinst, (hipStream_t)stream));
  return 0;
}
int mpdata_courant_device(int64_t ncrms, int nx, int nz, const double* u, const double* w, const double* rho, const double* adz,
                          double* clev, double* cinst, void* stream) {
  return courant_array(ncrms, nx, nz, u, w, rho, adz, clev, cinst, stream, 8);
}
int mpdata_courant_f32_device(int64_t ncrms, int nx, int nz, const float* u, const float* w, const float* rho, const float* adz,
                              float* clev, float* cinst, void* stream) {
  return courant_array(ncrms, nx, nz, u, w, rho, adz, clev, cinst, stream, 4);
}

// ---- 3i: per-level increments of f, in place.  Reads d, rewrites f on every column slot of the block's instances: no
// flag of the plan is touched and no event is recorded.  The hidden invariants hold by construction, not by a refresh:
//   halo marks  the increment is uniform in i, so halo columns that are wrapped copies stay wrapped copies (same bits in,
//               same operation) and stale ones stay stale -- halo_ok is right as it stands;
//   seam marks  every level a window stores takes the increment of the tall level it stands for, so fresh seams stay
//               fresh and stale ones stay stale -- seam_ok is right as it stands;
//   phantom     follows the plan's last instance inside the kernel (mpdata_level_add.h).
// A windowed plan's inner plan is rewritten where it lies (its stream and boundary are not forwarded: nothing of it runs).
static int plan_level_add(mpdata_plan* p, int64_t sl0, int64_t n, const void* d, int mode, int first, int count) {
  const int clip = mode == MPDATA_LEVEL_ADD_CLIP;
  if (plan_walked(p)) {
    MpdataLevelAddJob b;
    b.j = wm_job(wm_plan(p), 0, nullptr, first, count);
    b.sel = block_sel(p, sl0, n);
    b.d = d; b.clip = clip;
    HIP_TRY(mpdata_level_add_wm(b, p->stream));
  } else {
    HIP_TRY(mpdata_level_add_ref(ref_f(p, first), p->eb, p->ncrms, sl0, n, p->nx, p->nz - 1, count, d, clip, p->stream));
  }
  return 0;
}
static int plan_level_add_check(const char* what, const mpdata_plan* p, int64_t sl0, int64_t n, const void* d, int mode, int first,
                                int count, int eb) {
  int rc = block_ranges(what, p, sl0, n, first, count, eb);
  if (rc) return rc;
  if (!d) return set_err(MPDATA_EINVAL, "%s: null d", what);
  rc = level_add_mode(what, mode);
  return rc ? rc : plan_state(what, p, eb);
}
int mpdata_plan_level_add_device(mpdata_plan* p, int64_t sl0, int64_t n, const void* d, int mode, int first_tracer, int ntracers) {
  const int rc = plan_level_add_check("mpdata_plan_level_add_device", p, sl0, n, d, mode, first_tracer, ntracers, 0);
  if (rc) return rc;
  DevGuard g(p->device);
  return plan_level_add(p, sl0, n, d, mode, first_tracer, ntracers);
}
static int plan_level_add_host(mpdata_plan* p, int64_t sl0, int64_t n, const void* d, int mode, int eb) {
  int rc = plan_level_add_check("mpdata_plan_level_add", p, sl0, n, d, mode, 0, 0, eb);
  if (rc) return rc;
  DevGuard g(p->device);
  HostArr a[1] = {{d, (size_t)n * (p->nz - 1) * p->ntracers * eb, false}};
  rc = stage_in(p, a);
  if (!rc) rc = plan_level_add(p, sl0, n, a[0].dev, mode, 0, p->ntracers);
  return rc ? rc : stage_out(p, a);
}
int mpdata_plan_level_add(mpdata_plan* p, int64_t sl0, int64_t n, const double* d, int mode) {
  return plan_level_add_host(p, sl0, n, d, mode, 8);
}
int mpdata_plan_level_add_f32(mpdata_plan* p, int64_t sl0, int64_t n, const float* d, int mode) {
  return plan_level_add_host(p, sl0, n, d, mode, 4);
}
// the same on a reference-layout device array (arguments checked before any device call)
static int level_add_array(int64_t ncrms, int nx, int nz, int ntracers, void* f, const void* d, int mode, void* stream, int eb) {
  int rc = array_sizes("mpdata_level_add_device", ncrms, nx, nz, &ntracers);
  if (rc) return rc;
  if (!f || !d) return set_err(MPDATA_EINVAL, "mpdata_level_add_device: null %s", !f ? "f" : "d");
  rc = level_add_mode("mpdata_level_add_device", mode);
  if (rc) return rc;
  HIP_TRY(mpdata_level_add_ref(f, eb, ncrms, 0, ncrms, nx, nz - 1, ntracers, d, mode == MPDATA_LEVEL_ADD_CLIP, (hipStream_t)stream));
  return 0;
}
int mpdata_level_add_device(int64_t ncrms, int nx, int nz, int ntracers, double* f, const double* d, int mode, void* stream) {
  return level_add_array(ncrms, nx, nz, ntracers, f, d, mode, stream, 8);
}
int mpdata_level_add_f32_device(int64_t ncrms, int nx, int nz, int ntracers, float* f, const float* d, int mode, void* stream) {
  return level_add_array(ncrms, nx, nz, ntracers, f, d, mode, stream, 4);
}

// ---- 3j: one factor per instance on the plan's u and / or w, in place.  Reads su, sw, rewrites every column and level
// the plan stores of the block's instances: no flag of the plan is touched and no event is recorded.  f, flux, rho, rhow,
// adz are not looked at, so halo and seam marks are right as they stand; every window of an instance and every level it
// stores takes the instance's factor, so all stored copies of a tall level change alike; the phantom half follows the
// plan's last instance inside the kernel (mpdata_scale_uw.h).  A windowed plan's inner plan is rewritten where it lies.
static int plan_scale_uw(mpdata_plan* p, int64_t sl0, int64_t n, const void* su, const void* sw) {
  if (plan_walked(p)) {
    const mpdata_plan* q = wm_plan(p);
    MpdataScaleUwJob b;
    b.sel = block_sel(p, sl0, n);
    if (su) { b.j = wm_job(q, 1, nullptr, 0, 1); b.s = su; HIP_TRY(mpdata_scale_uw_wm(b, p->stream)); }
    if (sw) { b.j = wm_job(q, 2, nullptr, 0, 1); b.s = sw; HIP_TRY(mpdata_scale_uw_wm(b, p->stream)); }
  } else {
    if (su) HIP_TRY(mpdata_scale_uw_ref(p->u, p->eb, p->ncrms, sl0, n, p->nx + 5, p->nz - 1, su, p->stream));
    if (sw) HIP_TRY(mpdata_scale_uw_ref(p->w, p->eb, p->ncrms, sl0, n, p->nx + 4, p->nz, sw, p->stream));
  }
  return 0;
}
static int plan_scale_uw_check(const char* what, const mpdata_plan* p, int64_t sl0, int64_t n, const void* su, const void* sw, int eb) {
  const int rc = block_range(what, p, sl0, n);
  if (rc) return rc;
  if (!su && !sw) return set_err(MPDATA_EINVAL, "%s: su and sw are both NULL", what);
  return plan_state(what, p, eb, su != nullptr, sw != nullptr);
}
int mpdata_plan_scale_uw_device(mpdata_plan* p, int64_t sl0, int64_t n, const void* su, const void* sw) {
  const int rc = plan_scale_uw_check("mpdata_plan_scale_uw_device", p, sl0, n, su, sw, 0);
  if (rc) return rc;
  DevGuard g(p->device);
  return plan_scale_uw(p, sl0, n, su, sw);
}
static int plan_scale_uw_host(mpdata_plan* p, int64_t sl0, int64_t n, const void* su, const void* sw, int eb) {
  int rc = plan_scale_uw_check("mpdata_plan_scale_uw", p, sl0, n, su, sw, eb);
  if (rc) return rc;
  DevGuard g(p->device);
  HostArr a[2] = {{su, (size_t)n * eb, false}, {sw, (size_t)n * eb, false}};
  rc = stage_in(p, a);
  if (!rc) rc = plan_scale_uw(p, sl0, n, a[0].dev, a[1].dev);
  return rc ? rc : stage_out(p, a);
}
int mpdata_plan_scale_uw(mpdata_plan* p, int64_t sl0, int64_t n, const double* su, const double* sw) {
  return plan_scale_uw_host(p, sl0, n, su, sw, 8);
}
int mpdata_plan_scale_uw_f32(mpdata_plan* p, int64_t sl0, int64_t n, const float* su, const float* sw) {
  return plan_scale_uw_host(p, sl0, n, su, sw, 4);
}
// the same on reference-layout device arrays (arguments checked before any device call)
static int scale_uw_array(int64_t ncrms, int nx, int nz, void* u, void* w, const void* su, const void* sw, void* stream, int eb) {
  const int rc = array_sizes("mpdata_scale_uw_device", ncrms, nx, nz, nullptr);
  if (rc) return rc;
  if (!u && !w) return set_err(MPDATA_EINVAL, "mpdata_scale_uw_device: u and w are both NULL");
  if (!u != !su || !w != !sw)
    return set_err(MPDATA_EINVAL, "mpdata_scale_uw_device: %s without %s", !u != !su ? (u ? "u" : "su") : (w ? "w" : "sw"),
                   !u != !su ? (u ? "su" : "u") : (w ? "sw" : "w"));
  if (u) HIP_TRY(mpdata_scale_uw_ref(u, eb, ncrms, 0, ncrms, nx + 5, nz - 1, su, (hipStream_t)stream));
  if (w) HIP_TRY(mpdata_scale_uw_ref(w, eb, ncrms, 0, ncrms, nx + 4, nz, sw, (hipStream_t)stream));
  return 0;
}
int mpdata_scale_uw_device(int64_t ncrms, int nx, int nz, double* u, double* w, const double* su, const double* sw, void* stream) {
  return scale_uw_array(ncrms, nx, nz, u, w, su, sw, stream, 8);
}
int mpdata_scale_uw_f32_device(int64_t ncrms, int nx, int nz, float* u, float* w, const float* su, const float* sw, void* stream) {
  return scale_uw_array(ncrms, nx, nz, u, w, su, sw, stream, 4);
}

// ---- 3k: mass-weighted column integrals of f per interior column (path) and their sum over the columns (mass).  Reads f,
// rho, adz, writes the outputs: as the level statistics no flag of the plan is touched (halo columns are not read, owned
// levels are right whatever the seams hold), no event is recorded, and a windowed plan's inner plan is read where it
// lies.  The velocities are not looked at: the plan need not hold any.
static int plan_column_path(mpdata_plan* p, int64_t sl0, int64_t n, void* path, void* mass, int first, int count) {
  if (plan_walked(p)) {
    const mpdata_plan* q = wm_plan(p);
    MpdataColumnPathJob b;
    b.j = wm_job(q, 0, nullptr, first, count);
    kc_rho_adz(q, b);
    b.sel = block_sel(p, sl0, n);
    b.path = path; b.mass = mass;
    HIP_TRY(mpdata_column_path_wm(b, p->stream));
  } else {
    HIP_TRY(mpdata_column_path_ref(ref_f(p, first), p->rho, p->adz, p->eb, p->ncrms, sl0, n, p->nx, p->nz - 1, count, path, mass,
                                   p->stream));
  }
  return 0;
}
static int plan_column_path_check(const char* what, const mpdata_plan* p, int64_t sl0, int64_t n, const void* path, int first,
                                  int count, int eb) {
  const int rc = block_ranges(what, p, sl0, n, first, count, eb);
  if (rc) return rc;
  if (!path) return set_err(MPDATA_EINVAL, "%s: null path", what);
  return plan_state(what, p, eb);
}
int mpdata_plan_column_path_device(mpdata_plan* p, int64_t sl0, int64_t n, void* path, void* mass, int first_tracer, int ntracers) {
  const int rc = plan_column_path_check("mpdata_plan_column_path_device", p, sl0, n, path, first_tracer, ntracers, 0);
  if (rc) return rc;
  DevGuard g(p->device);
  return plan_column_path(p, sl0, n, path, mass, first_tracer, ntracers);
}
static int plan_column_path_host(mpdata_plan* p, int64_t sl0, int64_t n, void* path, void* mass, int eb) {
  int rc = plan_column_path_check("mpdata_plan_column_path", p, sl0, n, path, 0, 0, eb);
  if (rc) return rc;
  DevGuard g(p->device);
  HostArr a[2] = {{path, (size_t)n * p->nx * p->ntracers * eb, true}, {mass, (size_t)n * p->ntracers * eb, true}};
  rc = stage_in(p, a);
  if (!rc) rc = plan_column_path(p, sl0, n, a[0].dev, a[1].dev, 0, p->ntracers);
  return rc ? rc : stage_out(p, a);
}
int mpdata_plan_column_path(mpdata_plan* p, int64_t sl0, int64_t n, double* path, double* mass) {
  return plan_column_path_host(p, sl0, n, path, mass, 8);
}
int mpdata_plan_column_path_f32(mpdata_plan* p, int64_t sl0, int64_t n, float* path, float* mass) {
  return plan_column_path_host(p, sl0, n, path, mass, 4);
}
// the same on reference-layout device arrays (arguments checked before any device call)
static int column_path_array(int64_t ncrms, int nx, int nz, int ntracers, const void* f, const void* rho, const void* adz, void* path,
                             void* mass, void* stream, int eb) {
  const int rc = array_sizes("mpdata_column_path_device", ncrms, nx, nz, &ntracers);
  if (rc) return rc;
  if (!f || !rho || !adz) return set_err(MPDATA_EINVAL, "mpdata_column_path_device: null %s", !f ? "f" : !rho ? "rho" : "adz");
  if (!path) return set_err(MPDATA_EINVAL, "mpdata_column_path_device: null path");
  HIP_TRY(mpdata_column_path_ref(f, rho, adz, eb, ncrms, 0, ncrms, nx, nz - 1, ntracers, path, mass, (hipStream_t)stream));
  return 0;
}
int mpdata_column_path_device(int64_t ncrms, int nx, int nz, int ntracers, const double* f, const double* rho, const double* adz,
                              double* path, double* mass, void* stream) {
  return column_path_array(ncrms, nx, nz, ntracers, f, rho, adz, path, mass, stream, 8);
}
int mpdata_column_path_f32_device(int64_t ncrms, int nx, int nz, int ntracers, const float* f, const float* rho, const float* adz,
                                  float* path, float* mass, void* stream) {
  return column_path_array(ncrms, nx, nz, ntracers, f, rho, adz, path, mass, stream, 4);
}

// ---- 3l: eddy diffusion of f, in place.  Reads tkh, cx, cz, sb, st and the plan's rho and adz, rewrites the interior
// columns of f of the block's instances and the tracer range; flux, u, w, rho, rhow, adz and the boundary mode are not
// touched and no event is recorded.  The halo columns 0 and nx+1 are inputs: a periodic plan wraps stale halos first, as a
// run does, and afterwards its halos are copies of the OLD interior, so the marks of the range are cleared and the next
// run or read-back wraps again.  Wave-major plans: tkh is brought into the plan layout once per call by the conversion
// kernels of an import of f -- the block's for a block, the whole import's for the whole plan -- (a job of nx + 2 columns
// at column slot 2 into the plan's diffusion buffer; slots outside the block are not written and reach no result); reference-layout plans: the buffer takes the new interior (mpdata_diffuse.h).
static int plan_diffuse(mpdata_plan* p, int64_t sl0, int64_t n, const void* tkh, const void* cx, const void* cz, const void* sb,
                        const void* st, void* zflux, int first, int count) {
  const int nx = p->nx, nzm = p->nz - 1;
  const bool wm = p->layout == MPDATA_LAYOUT_WAVEMAJOR;
  int rc = plan_dbuf(p, wm ? (size_t)p->ntiles * p->tile_elems * 8 : (size_t)n * nx * nzm * count * p->eb);
  if (!rc) rc = plan_wrap_f(p, first, count);
  if (rc) return rc;
  if (wm) {
    MpdataBlockJob tj = wm_block_job(p, 0, const_cast<void*>(tkh), sl0, n, 0, 1);
    tj.j.prv = p->dbuf; tj.j.ncols = nx + 2; tj.j.prv_col0 = 2; tj.j.ref_levmul = nx + 2; tj.j.ref_tstride = 0; tj.j.prv_tstride = 0;
    if (n != p->ncrms) {
      HIP_TRY(mpdata_layout_convert_block(tj, true, p->stream));
    } else if (p->odd) {   // the whole plan: the kernels of a whole import of f (plan_import)
      HIP_TRY(mpdata_layout_convert_odd(&tj.j, 1, true, p->stream));
    } else if (!legacy_convert()) {
      const hipError_t e = mpdata_layout_import_rows(&tj.j, 1, p->stream);
      if (e == hipErrorNotSupported) HIP_TRY(mpdata_layout_convert_cols(&tj.j, 1, true, p->stream));
      else HIP_TRY(e);
    } else {
      HIP_TRY(mpdata_layout_convert(tj.j, 8, true, p->stream));
    }
    MpdataDiffuseJob b;
    b.j = wm_job(p, 0, nullptr, first, count);
    b.sel = block_sel(p, sl0, n);
    b.tkh = p->dbuf;
    kc_rho_adz(p, b);
    b.cx = cx; b.cz = cz; b.sb = sb; b.st = st; b.zflux = zflux;
    HIP_TRY(mpdata_diffuse_wm(b, p->stream));
  } else {
    HIP_TRY(mpdata_diffuse_ref(ref_f(p, first), p->rho, p->adz, p->eb, p->ncrms, sl0, n, nx, nzm, count, tkh, cx, cz, sb, st, zflux,
                               p->dbuf, p->stream));
  }
  return plan_rewrote(p, sl0, n, first, count, HALOS);
}
static int plan_diffuse_check(const char* what, const mpdata_plan* p, int64_t sl0, int64_t n, const void* tkh, const void* cx,
                              const void* cz, int first, int count, int eb) {
  const int rc = block_ranges(what, p, sl0, n, first, count, eb);
  if (rc) return rc;
  if (!tkh || !cx || !cz) return set_err(MPDATA_EINVAL, "%s: null %s", what, !tkh ? "tkh" : !cx ? "cx" : "cz");
  if (p->inner)
    return set_err(MPDATA_EUNSUPPORTED, "%s on a windowed plan (nz = %d > 238): tkh would have to be cut into level windows and the "
                                        "seams refreshed; not built yet", what, p->nz);
  return plan_state(what, p, eb);
}
int mpdata_plan_diffuse_device(mpdata_plan* p, int64_t sl0, int64_t n, const void* tkh, const void* cx, const void* cz, const void* sb,
                               const void* st, void* zflux, int first_tracer, int ntracers) {
  const int rc = plan_diffuse_check("mpdata_plan_diffuse_device", p, sl0, n, tkh, cx, cz, first_tracer, ntracers, 0);
  if (rc) return rc;
  DevGuard g(p->device);
  return plan_diffuse(p, sl0, n, tkh, cx, cz, sb, st, zflux, first_tracer, ntracers);
}
static int plan_diffuse_host(mpdata_plan* p, int64_t sl0, int64_t n, const void* tkh, const void* cx, const void* cz, const void* sb,
                             const void* st, void* zflux, int eb) {
  int rc = plan_diffuse_check("mpdata_plan_diffuse", p, sl0, n, tkh, cx, cz, 0, 0, eb);
  if (rc) return rc;
  DevGuard g(p->device);
  const size_t cb = (size_t)n * (p->nz - 1) * eb, xb = (size_t)n * p->nx * eb;
  HostArr a[6] = {{tkh, cb * (p->nx + 2), false}, {cx, cb, false}, {cz, cb, false}, {sb, xb, false}, {st, xb, false},
                  {zflux, (size_t)n * p->nz * p->ntracers * eb, true}};
  rc = stage_in(p, a);
  if (!rc) rc = plan_diffuse(p, sl0, n, a[0].dev, a[1].dev, a[2].dev, a[3].dev, a[4].dev, a[5].dev, 0, p->ntracers);
  return rc ? rc : stage_out(p, a);
}
int mpdata_plan_diffuse(mpdata_plan* p, int64_t sl0, int64_t n, const double* tkh, const double* cx, const double* cz, const double* sb,
                        const double* st, double* zflux) {
  return plan_diffuse_host(p, sl0, n, tkh, cx, cz, sb, st, zflux, 8);
}
int mpdata_plan_diffuse_f32(mpdata_plan* p, int64_t sl0, int64_t n, const float* tkh, const float* cx, const float* cz, const float* sb,
                            const float* st, float* zflux) {
  return plan_diffuse_host(p, sl0, n, tkh, cx, cz, sb, st, zflux, 4);
}
// the same on reference-layout device arrays (arguments checked before any device call).  The new interior of the block
// goes through a scratch array of the call's own, which is freed when the work is done: the call returns after it.
static int diffuse_array(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, void* f, const void* rho, const void* adz,
                         const void* tkh, const void* cx, const void* cz, const void* sb, const void* st, void* zflux, void* stream, int eb) {
  int rc = array_sizes("mpdata_diffuse_device", ncrms, nx, nz, &ntracers);
  if (rc) return rc;
  rc = array_block("mpdata_diffuse_device", ncrms, sl0, n);
  if (rc) return rc;
  if (!f || !rho || !adz) return set_err(MPDATA_EINVAL, "mpdata_diffuse_device: null %s", !f ? "f" : !rho ? "rho" : "adz");
  if (!tkh || !cx || !cz) return set_err(MPDATA_EINVAL, "mpdata_diffuse_device: null %s", !tkh ? "tkh" : !cx ? "cx" : "cz");
  void* scratch = nullptr;
  HIP_TRY(hipMalloc(&scratch, (size_t)n * nx * (nz - 1) * ntracers * eb));
  return scratch_done(scratch, stream, mpdata_diffuse_ref(f, rho, adz, eb, ncrms, sl0, n, nx, nz - 1, ntracers, tkh, cx, cz, sb, st, zflux,
                                                          scratch, (hipStream_t)stream));
}
int mpdata_diffuse_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, double* f, const double* rho,
                          const double* adz, const double* tkh, const double* cx, const double* cz, const double* sb, const double* st,
                          double* zflux, void* stream) {
  return diffuse_array(ncrms, nx, nz, ntracers, sl0, n, f, rho, adz, tkh, cx, cz, sb, st, zflux, stream, 8);
}
int mpdata_diffuse_f32_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, float* f, const float* rho,
                              const float* adz, const float* tkh, const float* cx, const float* cz, const float* sb, const float* st,
                              float* zflux, void* stream) {
  return diffuse_array(ncrms, nx, nz, ntracers, sl0, n, f, rho, adz, tkh, cx, cz, sb, st, zflux, stream, 4);
}

// ---- 3m: large-scale vertical advection of f, in place.  Reads cb, cc, rewrites f on every column slot of the block's
// instances and the tracer range; flux, u, w, rho, rhow, adz and the boundary mode are not touched and no event is recorded.
//   halo marks  the operator is the same in every column slot and couples none, so halo columns that are wrapped copies
//               stay wrapped copies (same bits in, same operations) and stale ones stay stale -- halo_ok is right as it stands;
//   seam marks  an owned level reads one level outside the owned range, so stale seams of the range are refreshed first,
//               as a run does; only owned levels are written, so afterwards the other copies are stale: the marks of the
//               range are cleared and the next run refreshes them;
//   phantom     follows the plan's last slot inside the kernel (mpdata_subside.h); on a windowed plan the refresh of the
//               inner plan follows as after a seam refresh.
// Reference-layout plans: the plan's diffusion buffer takes the new rows (mpdata_subside.h).
static int plan_subside(mpdata_plan* p, int64_t sl0, int64_t n, const void* cb, const void* cc, void* dsum, int first, int count) {
  if (plan_walked(p)) {
    const int rc = plan_seams(p, first, count);
    if (rc) return rc;
    MpdataSubsideJob b;
    b.j = wm_job(wm_plan(p), 0, nullptr, first, count);
    b.sel = block_sel(p, sl0, n);
    b.cb = cb; b.cc = cc; b.dsum = dsum;
    HIP_TRY(mpdata_subside_wm(b, p->stream));
  } else {
    const int rc = plan_dbuf(p, (size_t)n * (p->nx + 6) * (p->nz - 1) * count * p->eb);
    if (rc) return rc;
    HIP_TRY(mpdata_subside_ref(ref_f(p, first), p->eb, p->ncrms, sl0, n, p->nx, p->nz - 1, count, cb, cc, dsum, p->dbuf, p->stream));
  }
  return plan_rewrote(p, sl0, n, first, count, SEAMS);
}
static int plan_subside_check(const char* what, const mpdata_plan* p, int64_t sl0, int64_t n, const void* cb, const void* cc, int first,
                              int count, int eb) {
  const int rc = block_ranges(what, p, sl0, n, first, count, eb);
  if (rc) return rc;
  if (!cb || !cc) return set_err(MPDATA_EINVAL, "%s: null %s", what, !cb ? "cb" : "cc");
  return plan_state(what, p, eb);
}
int mpdata_plan_subside_device(mpdata_plan* p, int64_t sl0, int64_t n, const void* cb, const void* cc, void* dsum, int first_tracer,
                               int ntracers) {
  const int rc = plan_subside_check("mpdata_plan_subside_device", p, sl0, n, cb, cc, first_tracer, ntracers, 0);
  if (rc) return rc;
  DevGuard g(p->device);
  return plan_subside(p, sl0, n, cb, cc, dsum, first_tracer, ntracers);
}
static int plan_subside_host(mpdata_plan* p, int64_t sl0, int64_t n, const void* cb, const void* cc, void* dsum, int eb) {
  int rc = plan_subside_check("mpdata_plan_subside", p, sl0, n, cb, cc, 0, 0, eb);
  if (rc) return rc;
  DevGuard g(p->device);
  const size_t kb = (size_t)n * (p->nz - 1) * eb;
  HostArr a[3] = {{cb, kb, false}, {cc, kb, false}, {dsum, kb * p->ntracers, true}};
  rc = stage_in(p, a);
  if (!rc) rc = plan_subside(p, sl0, n, a[0].dev, a[1].dev, a[2].dev, 0, p->ntracers);
  return rc ? rc : stage_out(p, a);
}
int mpdata_plan_subside(mpdata_plan* p, int64_t sl0, int64_t n, const double* cb, const double* cc, double* dsum) {
  return plan_subside_host(p, sl0, n, cb, cc, dsum, 8);
}
int mpdata_plan_subside_f32(mpdata_plan* p, int64_t sl0, int64_t n, const float* cb, const float* cc, float* dsum) {
  return plan_subside_host(p, sl0, n, cb, cc, dsum, 4);
}
// the same on reference-layout device arrays (arguments checked before any device call).  The new rows go through a
// scratch array of the call's own, which is freed when the work is done: the call returns after it.
static int subside_array(int64_t ncrms, int nx, int nz, int ntracers, void* f, const void* cb, const void* cc, void* dsum, void* stream,
                         int eb) {
  const int rc = array_sizes("mpdata_subside_device", ncrms, nx, nz, &ntracers);
  if (rc) return rc;
  if (!f) return set_err(MPDATA_EINVAL, "mpdata_subside_device: null f");
  if (!cb || !cc) return set_err(MPDATA_EINVAL, "mpdata_subside_device: null %s", !cb ? "cb" : "cc");
  void* scratch = nullptr;
  HIP_TRY(hipMalloc(&scratch, (size_t)ncrms * (nx + 6) * (nz - 1) * ntracers * eb));
  return scratch_done(scratch, stream,
                      mpdata_subside_ref(f, eb, ncrms, 0, ncrms, nx, nz - 1, ntracers, cb, cc, dsum, scratch, (hipStream_t)stream));
}
int mpdata_subside_device(int64_t ncrms, int nx, int nz, int ntracers, double* f, const double* cb, const double* cc, double* dsum,
                          void* stream) {
  return subside_array(ncrms, nx, nz, ntracers, f, cb, cc, dsum, stream, 8);
}
int mpdata_subside_f32_device(int64_t ncrms, int nx, int nz, int ntracers, float* f, const float* cb, const float* cc, float* dsum,
                              void* stream) {
  return subside_array(ncrms, nx, nz, ntracers, f, cb, cc, dsum, stream, 4);
}

// ---- 3n: sedimentation of f, in place.  Reads wp and the plan's rho and adz, rewrites the INTERIOR columns of f of the
// block's instances and the tracer range; flux, u, w, rho, rhow, adz and the boundary mode are not touched and no event
// is recorded.
//   halo marks  halo columns are neither read nor written, so no wrap is launched in front; afterwards a periodic plan's
//               halos are copies of the OLD interior: the marks of the range are cleared and the next run or read-back
//               wraps again;
//   seam marks  an owned level reads the level above it, one level outside the owned range at a window's top, so stale
//               seams of the range are refreshed first, as a run does; only owned levels are written, so afterwards the
//               other copies are stale: the marks of the range are cleared and the next run refreshes them;
//   phantom     follows the plan's last slot inside the kernel (mpdata_sediment.h); on a windowed plan the refresh of the
//               inner plan follows as after a seam refresh.
// Wave-major and windowed plans: wp is read where it lies (mpdata_sediment.h), the diffusion buffer is not used.
// Reference-layout plans: the buffer takes the new interior.
static int plan_sediment(mpdata_plan* p, int64_t sl0, int64_t n, const void* wp, void* psfc, void* pflux, int first, int count) {
  if (plan_walked(p)) {
    const int rc = plan_seams(p, first, count);
    if (rc) return rc;
    const mpdata_plan* q = wm_plan(p);
    MpdataSedimentJob b;
    b.j = wm_job(q, 0, nullptr, first, count);
    kc_rho_adz(q, b);
    b.sel = block_sel(p, sl0, n);
    b.wp = wp; b.psfc = psfc; b.pflux = pflux;
    HIP_TRY(mpdata_sediment_wm(b, p->stream));
  } else {
    const int rc = plan_dbuf(p, (size_t)n * p->nx * (p->nz - 1) * count * p->eb);
    if (rc) return rc;
    HIP_TRY(mpdata_sediment_ref(ref_f(p, first), p->rho, p->adz, p->eb, p->ncrms, sl0, n, p->nx, p->nz - 1, count, wp, psfc, pflux,
                                p->dbuf, p->stream));
  }
  return plan_rewrote(p, sl0, n, first, count, SEAMS | HALOS);
}
static int plan_sediment_check(const char* what, const mpdata_plan* p, int64_t sl0, int64_t n, const void* wp, int first, int count,
                               int eb) {
  const int rc = block_ranges(what, p, sl0, n, first, count, eb);
  if (rc) return rc;
  if (!wp) return set_err(MPDATA_EINVAL, "%s: null wp", what);
  return plan_state(what, p, eb);
}
int mpdata_plan_sediment_device(mpdata_plan* p, int64_t sl0, int64_t n, const void* wp, void* psfc, void* pflux, int first_tracer,
                                int ntracers) {
  const int rc = plan_sediment_check("mpdata_plan_sediment_device", p, sl0, n, wp, first_tracer, ntracers, 0);
  if (rc) return rc;
  DevGuard g(p->device);
  return plan_sediment(p, sl0, n, wp, psfc, pflux, first_tracer, ntracers);
}
static int plan_sediment_host(mpdata_plan* p, int64_t sl0, int64_t n, const void* wp, void* psfc, void* pflux, int eb) {
  int rc = plan_sediment_check("mpdata_plan_sediment", p, sl0, n, wp, 0, 0, eb);
  if (rc) return rc;
  DevGuard g(p->device);
  const size_t xb = (size_t)n * p->nx * p->ntracers * eb, kb = (size_t)n * (p->nz - 1) * p->ntracers * eb;
  HostArr a[3] = {{wp, xb * (p->nz - 1), false}, {psfc, xb, true}, {pflux, kb, true}};
  rc = stage_in(p, a);
  if (!rc) rc = plan_sediment(p, sl0, n, a[0].dev, a[1].dev, a[2].dev, 0, p->ntracers);
  return rc ? rc : stage_out(p, a);
}
int mpdata_plan_sediment(mpdata_plan* p, int64_t sl0, int64_t n, const double* wp, double* psfc, double* pflux) {
  return plan_sediment_host(p, sl0, n, wp, psfc, pflux, 8);
}
int mpdata_plan_sediment_f32(mpdata_plan* p, int64_t sl0, int64_t n, const float* wp, float* psfc, float* pflux) {
  return plan_sediment_host(p, sl0, n, wp, psfc, pflux, 4);
}
// the same on reference-layout device arrays (arguments checked before any device call).  The new interior of the block
// goes through a scratch array of the call's own, which is freed when the work is done: the call returns after it.
static int sediment_array(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, void* f, const void* rho, const void* adz,
                          const void* wp, void* psfc, void* pflux, void* stream, int eb) {
  int rc = array_sizes("mpdata_sediment_device", ncrms, nx, nz, &ntracers);
  if (rc) return rc;
  rc = array_block("mpdata_sediment_device", ncrms, sl0, n);
  if (rc) return rc;
  if (!f || !rho || !adz) return set_err(MPDATA_EINVAL, "mpdata_sediment_device: null %s", !f ? "f" : !rho ? "rho" : "adz");
  if (!wp) return set_err(MPDATA_EINVAL, "mpdata_sediment_device: null wp");
  void* scratch = nullptr;
  HIP_TRY(hipMalloc(&scratch, (size_t)n * nx * (nz - 1) * ntracers * eb));
  return scratch_done(scratch, stream, mpdata_sediment_ref(f, rho, adz, eb, ncrms, sl0, n, nx, nz - 1, ntracers, wp, psfc, pflux, scratch,
                                                           (hipStream_t)stream));
}
int mpdata_sediment_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, double* f, const double* rho,
                           const double* adz, const double* wp, double* psfc, double* pflux, void* stream) {
  return sediment_array(ncrms, nx, nz, ntracers, sl0, n, f, rho, adz, wp, psfc, pflux, stream, 8);
}
int mpdata_sediment_f32_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, float* f, const float* rho,
                               const float* adz, const float* wp, float* psfc, float* pflux, void* stream) {
  return sediment_array(ncrms, nx, nz, ntracers, sl0, n, f, rho, adz, wp, psfc, pflux, stream, 4);
}

// ---- 3o: implicit vertical solve of f, in place.  Reads lo, di, up, rewrites the INTERIOR columns of f of the block's
// instances and the tracer range; flux, u, w, rho, rhow, adz and the boundary mode are not touched and no event is
// recorded.
//   halo marks  halo columns are neither read nor written, so no wrap is launched in front; afterwards a periodic plan's
//               halos are copies of the OLD interior: the marks of the range are cleared and the next run or read-back
//               wraps again;
//   seam marks  the recurrence reads and writes OWNED levels only, which are right whatever the seams hold (as the
//               column integrals of 3k argue): no refresh in front; afterwards the other copies are stale: the marks of
//               the range are cleared and the next run refreshes them;
//   phantom     follows the plan's last slot inside the kernel (mpdata_vsolve.h); on a windowed plan the kernel leaves it
//               alone and the refresh of the inner plan follows as after a seam refresh.
// Every kind of plan: a small kernel in front writes the factors p and g (2 n nzm reals) into the plan's diffusion buffer.
static int plan_vsolve(mpdata_plan* p, int64_t sl0, int64_t n, const void* lo, const void* di, const void* up, int first, int count) {
  const int nzm = p->nz - 1;
  const size_t kb = (size_t)n * nzm * p->eb;
  const int rc = plan_dbuf(p, 2 * kb);
  if (rc) return rc;
  void* const pf = p->dbuf;
  void* const gf = (char*)p->dbuf + kb;
  HIP_TRY(mpdata_vsolve_factor(lo, di, up, p->eb, n, nzm, pf, gf, p->stream));
  if (plan_walked(p)) {
    MpdataVsolveJob b;
    b.j = wm_job(wm_plan(p), 0, nullptr, first, count);
    b.sel = block_sel(p, sl0, n);
    b.lo = lo; b.pg = pf;
    HIP_TRY(mpdata_vsolve_wm(b, p->stream));
  } else {
    HIP_TRY(mpdata_vsolve_ref(ref_f(p, first), p->eb, p->ncrms, sl0, n, p->nx, nzm, count, lo, pf, gf, p->stream));
  }
  return plan_rewrote(p, sl0, n, first, count, SEAMS | HALOS);
}
static int plan_vsolve_check(const char* what, const mpdata_plan* p, int64_t sl0, int64_t n, const void* lo, const void* di,
                             const void* up, int first, int count, int eb) {
  const int rc = block_ranges(what, p, sl0, n, first, count, eb);
  if (rc) return rc;
  if (!lo || !di || !up) return set_err(MPDATA_EINVAL, "%s: null %s", what, !lo ? "lo" : !di ? "di" : "up");
  return plan_state(what, p, eb);
}
int mpdata_plan_vsolve_device(mpdata_plan* p, int64_t sl0, int64_t n, const void* lo, const void* di, const void* up, int first_tracer,
                              int ntracers) {
  const int rc = plan_vsolve_check("mpdata_plan_vsolve_device", p, sl0, n, lo, di, up, first_tracer, ntracers, 0);
  if (rc) return rc;
  DevGuard g(p->device);
  return plan_vsolve(p, sl0, n, lo, di, up, first_tracer, ntracers);
}
static int plan_vsolve_host(mpdata_plan* p, int64_t sl0, int64_t n, const void* lo, const void* di, const void* up, int eb) {
  int rc = plan_vsolve_check("mpdata_plan_vsolve", p, sl0, n, lo, di, up, 0, 0, eb);
  if (rc) return rc;
  DevGuard g(p->device);
  const size_t kb = (size_t)n * (p->nz - 1) * eb;
  HostArr a[3] = {{lo, kb, false}, {di, kb, false}, {up, kb, false}};
  rc = stage_in(p, a);
  if (!rc) rc = plan_vsolve(p, sl0, n, a[0].dev, a[1].dev, a[2].dev, 0, p->ntracers);
  return rc ? rc : stage_out(p, a);
}
int mpdata_plan_vsolve(mpdata_plan* p, int64_t sl0, int64_t n, const double* lo, const double* di, const double* up) {
  return plan_vsolve_host(p, sl0, n, lo, di, up, 8);
}
int mpdata_plan_vsolve_f32(mpdata_plan* p, int64_t sl0, int64_t n, const float* lo, const float* di, const float* up) {
  return plan_vsolve_host(p, sl0, n, lo, di, up, 4);
}
// the same on reference-layout device arrays (arguments checked before any device call).  The factors go through a
// scratch array of the call's own, which is freed when the work is done: the call returns after it.
static int vsolve_array(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, void* f, const void* lo, const void* di,
                        const void* up, void* stream, int eb) {
  int rc = array_sizes("mpdata_vsolve_device", ncrms, nx, nz, &ntracers);
  if (rc) return rc;
  rc = array_block("mpdata_vsolve_device", ncrms, sl0, n);
  if (rc) return rc;
  if (!f) return set_err(MPDATA_EINVAL, "mpdata_vsolve_device: null f");
  if (!lo || !di || !up) return set_err(MPDATA_EINVAL, "mpdata_vsolve_device: null %s", !lo ? "lo" : !di ? "di" : "up");
  const size_t kb = (size_t)n * (nz - 1) * eb;
  void* scratch = nullptr;
  HIP_TRY(hipMalloc(&scratch, 2 * kb));
  void* const gf = (char*)scratch + kb;
  hipError_t e = mpdata_vsolve_factor(lo, di, up, eb, n, nz - 1, scratch, gf, (hipStream_t)stream);
  if (e == hipSuccess) e = mpdata_vsolve_ref(f, eb, ncrms, sl0, n, nx, nz - 1, ntracers, lo, scratch, gf, (hipStream_t)stream);
  return scratch_done(scratch, stream, e);
}
int mpdata_vsolve_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, double* f, const double* lo,
                         const double* di, const double* up, void* stream) {
  return vsolve_array(ncrms, nx, nz, ntracers, sl0, n, f, lo, di, up, stream, 8);
}
int mpdata_vsolve_f32_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, float* f, const float* lo,
                             const float* di, const float* up, void* stream) {
  return vsolve_array(ncrms, nx, nz, ntracers, sl0, n, f, lo, di, up, stream, 4);
}

// ---- 3p: per-cell sources of f, in place.  Reads s, rewrites the INTERIOR columns of f of the block's instances and the
// tracer range; flux, u, w, rho, rhow, adz and the boundary mode are not touched and no event is recorded.
//   halo marks  halo columns are neither read nor written, so no wrap is launched in front; afterwards a periodic plan's
//               halos are copies of the OLD interior: the marks of the range are cleared and the next run or read-back
//               wraps again;
//   seam marks  the operator is pointwise and reads and writes OWNED levels only, which are right whatever the seams
//               hold: no refresh in front; afterwards the other copies are stale: the marks of the range are cleared and
//               the next run refreshes them;
//   phantom     follows the plan's last slot inside the kernel (mpdata_cell_add.h); on a windowed plan the refresh of the
//               inner plan follows as after a seam refresh.
// Every kind of plan: s is read where it lies and f is updated in place; the diffusion buffer is not used.
static int plan_cell_add(mpdata_plan* p, int64_t sl0, int64_t n, const void* s, double c, int mode, void* dsum, int first, int count) {
  const int clip = mode == MPDATA_CELL_ADD_CLIP;
  if (plan_walked(p)) {
    MpdataCellAddJob b;
    b.j = wm_job(wm_plan(p), 0, nullptr, first, count);
    b.sel = block_sel(p, sl0, n);
    b.s = s; b.c = c; b.clip = clip; b.dsum = dsum;
    HIP_TRY(mpdata_cell_add_wm(b, p->stream));
  } else {
    HIP_TRY(mpdata_cell_add_ref(ref_f(p, first), p->eb, p->ncrms, sl0, n, p->nx, p->nz - 1, count, s, c, clip, dsum, p->stream));
  }
  return plan_rewrote(p, sl0, n, first, count, SEAMS | HALOS);
}
static int plan_cell_add_check(const char* what, const mpdata_plan* p, int64_t sl0, int64_t n, const void* s, int mode, int first,
                               int count, int eb) {
  int rc = block_ranges(what, p, sl0, n, first, count, eb);
  if (rc) return rc;
  if (!s) return set_err(MPDATA_EINVAL, "%s: null s", what);
  rc = cell_add_mode(what, mode);
  return rc ? rc : plan_state(what, p, eb);
}
int mpdata_plan_cell_add_device(mpdata_plan* p, int64_t sl0, int64_t n, const void* s, double c, int mode, void* dsum, int first_tracer,
                                int ntracers) {
  const int rc = plan_cell_add_check("mpdata_plan_cell_add_device", p, sl0, n, s, mode, first_tracer, ntracers, 0);
  if (rc) return rc;
  DevGuard g(p->device);
  return plan_cell_add(p, sl0, n, s, c, mode, dsum, first_tracer, ntracers);
}
static int plan_cell_add_host(mpdata_plan* p, int64_t sl0, int64_t n, const void* s, double c, int mode, void* dsum, int eb) {
  int rc = plan_cell_add_check("mpdata_plan_cell_add", p, sl0, n, s, mode, 0, 0, eb);
  if (rc) return rc;
  DevGuard g(p->device);
  const size_t kb = (size_t)n * (p->nz - 1) * p->ntracers * eb;
  HostArr a[2] = {{s, kb * p->nx, false}, {dsum, kb, true}};
  rc = stage_in(p, a);
  if (!rc) rc = plan_cell_add(p, sl0, n, a[0].dev, c, mode, a[1].dev, 0, p->ntracers);
  return rc ? rc : stage_out(p, a);
}
int mpdata_plan_cell_add(mpdata_plan* p, int64_t sl0, int64_t n, const double* s, double c, int mode, double* dsum) {
  return plan_cell_add_host(p, sl0, n, s, c, mode, dsum, 8);
}
int mpdata_plan_cell_add_f32(mpdata_plan* p, int64_t sl0, int64_t n, const float* s, float c, int mode, float* dsum) {
  return plan_cell_add_host(p, sl0, n, s, (double)c, mode, dsum, 4);
}
// the same on reference-layout device arrays (arguments checked before any device call): in place, asynchronous
static int cell_add_array(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, void* f, const void* s, double c, int mode,
                          void* dsum, void* stream, int eb) {
  int rc = array_sizes("mpdata_cell_add_device", ncrms, nx, nz, &ntracers);
  if (rc) return rc;
  rc = array_block("mpdata_cell_add_device", ncrms, sl0, n);
  if (rc) return rc;
  if (!f) return set_err(MPDATA_EINVAL, "mpdata_cell_add_device: null f");
  if (!s) return set_err(MPDATA_EINVAL, "mpdata_cell_add_device: null s");
  rc = cell_add_mode("mpdata_cell_add_device", mode);
  if (rc) return rc;
  HIP_TRY(mpdata_cell_add_ref(f, eb, ncrms, sl0, n, nx, nz - 1, ntracers, s, c, mode == MPDATA_CELL_ADD_CLIP, dsum, (hipStream_t)stream));
  return 0;
}
int mpdata_cell_add_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, double* f, const double* s, double c,
                           int mode, double* dsum, void* stream) {
  return cell_add_array(ncrms, nx, nz, ntracers, sl0, n, f, s, c, mode, dsum, stream, 8);
}
int mpdata_cell_add_f32_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, float* f, const float* s, float c,
                               int mode, float* dsum, void* stream) {
  return cell_add_array(ncrms, nx, nz, ntracers, sl0, n, f, s, (double)c, mode, dsum, stream, 4);
}

// ---- 3q: the fused column step of f, in place: source, subside, sediment, vsolve in this order, each stage present with
// its arrays.  Rewrites the INTERIOR columns of f of the block's instances and the tracer range; flux, u, w, rho, rhow, adz
// and the boundary mode are not touched and no event is recorded.
//   halo marks  halo columns are neither read nor written (3m alone also updates them: the one difference from the
//               sequence of single calls besides the horizontal sums), so no wrap is launched in front; afterwards a
//               periodic plan's halos are copies of an OLD interior: the marks of the range are cleared and the next run or
//               read-back wraps again;
//   windowed    refused in the check: stages 2 and 3 need fresh seams of the field stage 1 leaves, stage 4 crosses the
//               windows twice;
//   phantom     follows the plan's last slot inside the kernel (mpdata_column_step.h).
// With stage 4 a small kernel in front writes the factors p and g (2 n nzm reals) into the plan's diffusion buffer, as 3o;
// with stage 3 on a wave-major plan another writes 1 / (rho * adz) (n nzm reals) behind them.
struct ColumnStepArgs {
  const void* s; double c; int mode;
  const void *cb, *cc, *wp; void* psfc;
  const void *lo, *di, *up;
};
static int plan_column_step(mpdata_plan* p, int64_t sl0, int64_t n, const ColumnStepArgs& x, int first, int count) {
  const int nzm = p->nz - 1;
  MpdataColumnStepArrays a;
  a.s = x.s; a.c = x.c; a.clip = x.s && x.mode == MPDATA_CELL_ADD_CLIP;
  a.cb = x.cb; a.cc = x.cc; a.wp = x.wp; a.psfc = x.psfc; a.lo = x.lo; a.pg = nullptr;
  const size_t kb = (size_t)n * nzm * p->eb;   // the diffusion buffer: p, g, then 1 / (rho * adz) of a plan-layout call
  if (x.lo || (x.wp && plan_walked(p))) {
    const int rc = plan_dbuf(p, 3 * kb);
    if (rc) return rc;
  }
  if (x.lo) {
    HIP_TRY(mpdata_vsolve_factor(x.lo, x.di, x.up, p->eb, n, nzm, p->dbuf, (char*)p->dbuf + kb, p->stream));
    a.pg = p->dbuf;
  }
  if (plan_walked(p)) {
    MpdataColumnStepJob b;
    b.j = wm_job(p, 0, nullptr, first, count);
    kc_rho_adz(p, b);
    b.sel = block_sel(p, sl0, n);
    b.ir = x.wp ? (char*)p->dbuf + 2 * kb : nullptr;
    b.a = a;
    HIP_TRY(mpdata_column_step_wm(b, p->stream));
  } else {
    HIP_TRY(mpdata_column_step_ref(ref_f(p, first), p->rho, p->adz, p->eb, p->ncrms, sl0, n, p->nx, nzm, count, a, p->stream));
  }
  return plan_rewrote(p, sl0, n, first, count, HALOS);
}
// the NULLs and the mode of a call, for the plan forms and the array forms alike
static int column_step_stages(const char* what, const ColumnStepArgs& x) {
  const int nv = (x.lo != nullptr) + (x.di != nullptr) + (x.up != nullptr);
  if (!x.s && !x.cb && !x.cc && !x.wp && !nv && !x.psfc) return set_err(MPDATA_EINVAL, "%s: no stage present (s, cb and cc, wp, lo di up are all NULL)", what);
  if (!x.cb != !x.cc) return set_err(MPDATA_EINVAL, "%s: %s without %s", what, x.cb ? "cb" : "cc", x.cb ? "cc" : "cb");
  if (nv == 1 || nv == 2) return set_err(MPDATA_EINVAL, "%s: null %s (lo, di and up go together)", what, !x.lo ? "lo" : !x.di ? "di" : "up");
  if (x.psfc && !x.wp) return set_err(MPDATA_EINVAL, "%s: psfc without wp", what);
  return x.s ? cell_add_mode(what, x.mode) : 0;
}
static int plan_column_step_check(const char* what, const mpdata_plan* p, int64_t sl0, int64_t n, const ColumnStepArgs& x, int first,
                                  int count, int eb) {
  int rc = block_ranges(what, p, sl0, n, first, count, eb);
  if (rc) return rc;
  rc = column_step_stages(what, x);
  if (rc) return rc;
  if (p->inner)
    return set_err(MPDATA_EUNSUPPORTED, "%s on a windowed plan (nz = %d > 238): the stages would need the seams refreshed between "
                                        "them; not built yet -- use the single calls", what, p->nz);
  return plan_state(what, p, eb);
}
int mpdata_plan_column_step_device(mpdata_plan* p, int64_t sl0, int64_t n, const void* s, double c, int mode, const void* cb,
                                   const void* cc, const void* wp, void* psfc, const void* lo, const void* di, const void* up,
                                   int first_tracer, int ntracers) {
  const ColumnStepArgs x = {s, c, mode, cb, cc, wp, psfc, lo, di, up};
  const int rc = plan_column_step_check("mpdata_plan_column_step_device", p, sl0, n, x, first_tracer, ntracers, 0);
  if (rc) return rc;
  DevGuard g(p->device);
  return plan_column_step(p, sl0, n, x, first_tracer, ntracers);
}
static int plan_column_step_host(mpdata_plan* p, int64_t sl0, int64_t n, const ColumnStepArgs& x, int eb) {
  int rc = plan_column_step_check("mpdata_plan_column_step", p, sl0, n, x, 0, 0, eb);
  if (rc) return rc;
  DevGuard g(p->device);
  const size_t kb = (size_t)n * (p->nz - 1) * eb, xb = (size_t)n * p->nx * p->ntracers * eb;
  HostArr a[8] = {{x.s, xb * (p->nz - 1), false}, {x.cb, kb, false}, {x.cc, kb, false}, {x.wp, xb * (p->nz - 1), false},
                  {x.psfc, xb, true}, {x.lo, kb, false}, {x.di, kb, false}, {x.up, kb, false}};
  rc = stage_in(p, a);
  const ColumnStepArgs d = {a[0].dev, x.c, x.mode, a[1].dev, a[2].dev, a[3].dev, a[4].dev, a[5].dev, a[6].dev, a[7].dev};
  if (!rc) rc = plan_column_step(p, sl0, n, d, 0, p->ntracers);
  return rc ? rc : stage_out(p, a);
}
int mpdata_plan_column_step(mpdata_plan* p, int64_t sl0, int64_t n, const double* s, double c, int mode, const double* cb,
                            const double* cc, const double* wp, double* psfc, const double* lo, const double* di, const double* up) {
  const ColumnStepArgs x = {s, c, mode, cb, cc, wp, psfc, lo, di, up};
  return plan_column_step_host(p, sl0, n, x, 8);
}
int mpdata_plan_column_step_f32(mpdata_plan* p, int64_t sl0, int64_t n, const float* s, float c, int mode, const float* cb,
                                const float* cc, const float* wp, float* psfc, const float* lo, const float* di, const float* up) {
  const ColumnStepArgs x = {s, (double)c, mode, cb, cc, wp, psfc, lo, di, up};
  return plan_column_step_host(p, sl0, n, x, 4);
}
// the same on reference-layout device arrays (arguments checked before any device call): in place.  Without stage 4 the
// call is asynchronous; with it the factors go through a scratch array of the call's own, which is freed when the work is
// done: the call returns after it.
static int column_step_array(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, void* f, const void* rho,
                             const void* adz, const ColumnStepArgs& x, void* stream, int eb) {
  const char* const what = "mpdata_column_step_device";
  int rc = array_sizes(what, ncrms, nx, nz, &ntracers);
  if (rc) return rc;
  rc = array_block(what, ncrms, sl0, n);
  if (rc) return rc;
  if (!f) return set_err(MPDATA_EINVAL, "%s: null f", what);
  rc = column_step_stages(what, x);
  if (rc) return rc;
  if (x.wp && (!rho || !adz)) return set_err(MPDATA_EINVAL, "%s: null %s (required with wp)", what, !rho ? "rho" : "adz");
  MpdataColumnStepArrays a;
  a.s = x.s; a.c = x.c; a.clip = x.s && x.mode == MPDATA_CELL_ADD_CLIP;
  a.cb = x.cb; a.cc = x.cc; a.wp = x.wp; a.psfc = x.psfc; a.lo = x.lo; a.pg = nullptr;
  if (!x.lo) {
    HIP_TRY(mpdata_column_step_ref(f, rho, adz, eb, ncrms, sl0, n, nx, nz - 1, ntracers, a, (hipStream_t)stream));
    return 0;
  }
  const size_t kb = (size_t)n * (nz - 1) * eb;
  void* scratch = nullptr;
  HIP_TRY(hipMalloc(&scratch, 2 * kb));
  a.pg = scratch;
  hipError_t e = mpdata_vsolve_factor(x.lo, x.di, x.up, eb, n, nz - 1, scratch, (char*)scratch + kb, (hipStream_t)stream);
  if (e == hipSuccess) e = mpdata_column_step_ref(f, rho, adz, eb, ncrms, sl0, n, nx, nz - 1, ntracers, a, (hipStream_t)stream);
  return scratch_done(scratch, stream, e);
}
int mpdata_column_step_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, double* f, const double* rho,
                              const double* adz, const double* s, double c, int mode, const double* cb, const double* cc,
                              const double* wp, double* psfc, const double* lo, const double* di, const double* up, void* stream) {
  const ColumnStepArgs x = {s, c, mode, cb, cc, wp, psfc, lo, di, up};
  return column_step_array(ncrms, nx, nz, ntracers, sl0, n, f, rho, adz, x, stream, 8);
}
int mpdata_column_step_f32_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, float* f, const float* rho,
                                  const float* adz, const float* s, float c, int mode, const float* cb, const float* cc,
                                  const float* wp, float* psfc, const float* lo, const float* di, const float* up, void* stream) {
  const ColumnStepArgs x = {s, (double)c, mode, cb, cc, wp, psfc, lo, di, up};
  return column_step_array(ncrms, nx, nz, ntracers, sl0, n, f, rho, adz, x, stream, 4);
}

// ---- 3r: relaxation of f to a level profile, in place: f = f - c * (f - m), m the given target or the horizontal mean of
// f.  Reads c and target, writes mean, rewrites the INTERIOR columns of f of the block's instances and the tracer range;
// flux, u, w, rho, rhow, adz and the boundary mode are not touched and no event is recorded.
//   halo marks  halo columns are neither read nor written, so no wrap is launched in front; afterwards a periodic plan's
//               halos are copies of the OLD interior: the marks of the range are cleared and the next run or read-back
//               wraps again;
//   seam marks  given m the operator is pointwise, and m is formed from the owned level's own columns: the call reads
//               and writes OWNED levels only, which are right whatever the seams hold: no refresh in front; afterwards the
//               other copies are stale: the marks of the range are cleared and the next run refreshes them;
//   phantom     follows the plan's last slot inside the kernel (mpdata_relax.h); on a windowed plan the refresh of the
//               inner plan follows as after a seam refresh.
// Every kind of plan: c and target are read where they lie and f is updated in place; the diffusion buffer is not used.
static int plan_relax(mpdata_plan* p, int64_t sl0, int64_t n, const void* c, const void* target, void* mean, int first, int count) {
  if (plan_walked(p)) {
    MpdataRelaxJob b;
    b.j = wm_job(wm_plan(p), 0, nullptr, first, count);
    b.sel = block_sel(p, sl0, n);
    b.c = c; b.target = target; b.mean = mean;
    HIP_TRY(mpdata_relax_wm(b, p->stream));
  } else {
    HIP_TRY(mpdata_relax_ref(ref_f(p, first), p->eb, p->ncrms, sl0, n, p->nx, p->nz - 1, count, c, target, mean, p->stream));
  }
  return plan_rewrote(p, sl0, n, first, count, SEAMS | HALOS);
}
static int plan_relax_check(const char* what, const mpdata_plan* p, int64_t sl0, int64_t n, const void* c, int first, int count, int eb) {
  const int rc = block_ranges(what, p, sl0, n, first, count, eb);
  if (rc) return rc;
  if (!c) return set_err(MPDATA_EINVAL, "%s: null c", what);
  return plan_state(what, p, eb);
}
int mpdata_plan_relax_device(mpdata_plan* p, int64_t sl0, int64_t n, const void* c, const void* target, void* mean, int first_tracer,
                             int ntracers) {
  const int rc = plan_relax_check("mpdata_plan_relax_device", p, sl0, n, c, first_tracer, ntracers, 0);
  if (rc) return rc;
  DevGuard g(p->device);
  return plan_relax(p, sl0, n, c, target, mean, first_tracer, ntracers);
}
static int plan_relax_host(mpdata_plan* p, int64_t sl0, int64_t n, const void* c, const void* target, void* mean, int eb) {
  int rc = plan_relax_check("mpdata_plan_relax", p, sl0, n, c, 0, 0, eb);
  if (rc) return rc;
  DevGuard g(p->device);
  const size_t kb = (size_t)n * (p->nz - 1) * eb;
  HostArr a[3] = {{c, kb, false}, {target, kb * p->ntracers, false}, {mean, kb * p->ntracers, true}};
  rc = stage_in(p, a);
  if (!rc) rc = plan_relax(p, sl0, n, a[0].dev, a[1].dev, a[2].dev, 0, p->ntracers);
  return rc ? rc : stage_out(p, a);
}
int mpdata_plan_relax(mpdata_plan* p, int64_t sl0, int64_t n, const double* c, const double* target, double* mean) {
  return plan_relax_host(p, sl0, n, c, target, mean, 8);
}
int mpdata_plan_relax_f32(mpdata_plan* p, int64_t sl0, int64_t n, const float* c, const float* target, float* mean) {
  return plan_relax_host(p, sl0, n, c, target, mean, 4);
}
// the same on reference-layout device arrays (arguments checked before any device call): in place, asynchronous
static int relax_array(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, void* f, const void* c, const void* target,
                       void* mean, void* stream, int eb) {
  int rc = array_sizes("mpdata_relax_device", ncrms, nx, nz, &ntracers);
  if (rc) return rc;
  rc = array_block("mpdata_relax_device", ncrms, sl0, n);
  if (rc) return rc;
  if (!f) return set_err(MPDATA_EINVAL, "mpdata_relax_device: null f");
  if (!c) return set_err(MPDATA_EINVAL, "mpdata_relax_device: null c");
  HIP_TRY(mpdata_relax_ref(f, eb, ncrms, sl0, n, nx, nz - 1, ntracers, c, target, mean, (hipStream_t)stream));
  return 0;
}
int mpdata_relax_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, double* f, const double* c,
                        const double* target, double* mean, void* stream) {
  return relax_array(ncrms, nx, nz, ntracers, sl0, n, f, c, target, mean, stream, 8);
}
int mpdata_relax_f32_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, float* f, const float* c,
                            const float* target, float* mean, void* stream) {
  return relax_array(ncrms, nx, nz, ntracers, sl0, n, f, c, target, mean, stream, 4);
}

// ---- 3s: implicit vertical diffusion of f with a per-cell diffusivity, in place.  Reads tkh, cz, sb, st and the plan's rho
// and adz, rewrites the INTERIOR columns of f of the block's instances and the tracer range; flux, u, w, rho, rhow, adz and
// the boundary mode are not touched and no event is recorded.
//   halo marks  halo columns are neither read nor written, so no wrap is launched in front; afterwards a periodic plan's
//               halos are copies of the OLD interior: the marks of the range are cleared and the next run or read-back
//               wraps again;
//   windowed    refused in the check: the backward sweep needs g of every cell of the windows below, which a second pass
//               would have to park in device memory;
//   phantom     follows the plan's last slot inside the kernel (mpdata_vdiffuse.h).
// Wave-major plans: tkh is read where it lies; a small kernel in front writes 1 / (rho * adz) (n nzm reals) into the plan's
// diffusion buffer.  Reference-layout plans: the buffer takes g of every cell of the block (n nx nzm reals).
static int plan_vdiffuse(mpdata_plan* p, int64_t sl0, int64_t n, const void* tkh, const void* cz, const void* sb, const void* st,
                         int first, int count) {
  const int nzm = p->nz - 1;
  const bool wm = plan_walked(p);
  const int rc = plan_dbuf(p, (size_t)n * nzm * p->eb * (wm ? 1 : p->nx));
  if (rc) return rc;
  if (wm) {
    MpdataVdiffuseJob b;
    b.j = wm_job(p, 0, nullptr, first, count);
    kc_rho_adz(p, b);
    b.sel = block_sel(p, sl0, n);
    b.ir = p->dbuf;
    b.tkh = tkh; b.cz = cz; b.sb = sb; b.st = st;
    HIP_TRY(mpdata_vdiffuse_wm(b, p->stream));
  } else {
    HIP_TRY(mpdata_vdiffuse_ref(ref_f(p, first), p->rho, p->adz, p->eb, p->ncrms, sl0, n, p->nx, nzm, count, tkh, cz, sb, st, p->dbuf,
                                p->stream));
  }
  return plan_rewrote(p, sl0, n, first, count, HALOS);
}
static int plan_vdiffuse_check(const char* what, const mpdata_plan* p, int64_t sl0, int64_t n, const void* tkh, const void* cz, int first,
                               int count, int eb) {
  const int rc = block_ranges(what, p, sl0, n, first, count, eb);
  if (rc) return rc;
  if (!tkh || !cz) return set_err(MPDATA_EINVAL, "%s: null %s", what, !tkh ? "tkh" : "cz");
  if (p->inner)
    return set_err(MPDATA_EUNSUPPORTED, "%s on a windowed plan (nz = %d > 238): the backward sweep needs g of every cell of the "
                                        "windows below, a second pass would have to park it; not built yet", what, p->nz);
  return plan_state(what, p, eb);
}
int mpdata_plan_vdiffuse_device(mpdata_plan* p, int64_t sl0, int64_t n, const void* tkh, const void* cz, const void* sb, const void* st,
                                int first_tracer, int ntracers) {
  const int rc = plan_vdiffuse_check("mpdata_plan_vdiffuse_device", p, sl0, n, tkh, cz, first_tracer, ntracers, 0);
  if (rc) return rc;
  DevGuard g(p->device);
  return plan_vdiffuse(p, sl0, n, tkh, cz, sb, st, first_tracer, ntracers);
}
static int plan_vdiffuse_host(mpdata_plan* p, int64_t sl0, int64_t n, const void* tkh, const void* cz, const void* sb, const void* st,
                              int eb) {
  int rc = plan_vdiffuse_check("mpdata_plan_vdiffuse", p, sl0, n, tkh, cz, 0, 0, eb);
  if (rc) return rc;
  DevGuard g(p->device);
  const size_t kb = (size_t)n * (p->nz - 1) * eb, xb = (size_t)n * p->nx * eb;
  HostArr a[4] = {{tkh, kb * (p->nx + 2), false}, {cz, kb, false}, {sb, xb, false}, {st, xb, false}};
  rc = stage_in(p, a);
  if (!rc) rc = plan_vdiffuse(p, sl0, n, a[0].dev, a[1].dev, a[2].dev, a[3].dev, 0, p->ntracers);
  return rc ? rc : stage_out(p, a);
}
int mpdata_plan_vdiffuse(mpdata_plan* p, int64_t sl0, int64_t n, const double* tkh, const double* cz, const double* sb,
                         const double* st) {
  return plan_vdiffuse_host(p, sl0, n, tkh, cz, sb, st, 8);
}
int mpdata_plan_vdiffuse_f32(mpdata_plan* p, int64_t sl0, int64_t n, const float* tkh, const float* cz, const float* sb, const float* st) {
  return plan_vdiffuse_host(p, sl0, n, tkh, cz, sb, st, 4);
}
// the same on reference-layout device arrays (arguments checked before any device call).  g of every cell of the block
// goes through a scratch array of the call's own, which is freed when the work is done: the call returns after it.
static int vdiffuse_array(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, void* f, const void* rho, const void* adz,
                          const void* tkh, const void* cz, const void* sb, const void* st, void* stream, int eb) {
  int rc = array_sizes("mpdata_vdiffuse_device", ncrms, nx, nz, &ntracers);
  if (rc) return rc;
  rc = array_block("mpdata_vdiffuse_device", ncrms, sl0, n);
  if (rc) return rc;
  if (!f || !rho || !adz) return set_err(MPDATA_EINVAL, "mpdata_vdiffuse_device: null %s", !f ? "f" : !rho ? "rho" : "adz");
  if (!tkh || !cz) return set_err(MPDATA_EINVAL, "mpdata_vdiffuse_device: null %s", !tkh ? "tkh" : "cz");
  void* scratch = nullptr;
  HIP_TRY(hipMalloc(&scratch, (size_t)n * nx * (nz - 1) * eb));
  return scratch_done(scratch, stream, mpdata_vdiffuse_ref(f, rho, adz, eb, ncrms, sl0, n, nx, nz - 1, ntracers, tkh, cz, sb, st, scratch,
                                                           (hipStream_t)stream));
}
int mpdata_vdiffuse_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, double* f, const double* rho,
                           const double* adz, const double* tkh, const double* cz, const double* sb, const double* st, void* stream) {
  return vdiffuse_array(ncrms, nx, nz, ntracers, sl0, n, f, rho, adz, tkh, cz, sb, st, stream, 8);
}
int mpdata_vdiffuse_f32_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, float* f, const float* rho,
                               const float* adz, const float* tkh, const float* cz, const float* sb, const float* st, void* stream) {
  return vdiffuse_array(ncrms, nx, nz, ntracers, sl0, n, f, rho, adz, tkh, cz, sb, st, stream, 4);
}

// ---- 3t: first-order conversion between two tracers of f, in place: d = r * max(a - q0, 0), capped by max(a, 0) on
// request, taken from tracer src and given (times y) to tracer dst.  Reads r, q0 and y, writes dsum, rewrites the INTERIOR
// columns of tracers src and dst of the block's instances; every other tracer, flux, u, w, rho, rhow, adz and the boundary
// mode are not touched and no event is recorded.
//   halo marks  halo columns are neither read nor written, so no wrap is launched in front; afterwards a periodic plan's
//               halos of BOTH tracers are copies of the OLD interior: their marks are cleared and the next run or
//               read-back wraps again;
//   seam marks  the operator is pointwise in (i, k): the call reads and writes OWNED levels only, which are right whatever
//               the seams hold: no refresh in front; afterwards the other copies of both tracers are stale: their marks are
//               cleared and the next run refreshes them;
//   phantom     follows the plan's last slot inside the kernel, in both tracers (mpdata_convert.h); on a windowed plan the
//               refresh of the inner plan follows as after a seam refresh.
// Every kind of plan: r, q0 and y are read where they lie and f is updated in place; the diffusion buffer is not used.
static int plan_convert(mpdata_plan* p, int64_t sl0, int64_t n, int src, int dst, const void* r, const void* q0, const void* y, int mode,
                        void* dsum) {
  const int limit = (mode & MPDATA_CONVERT_LIMIT) != 0;
  if (plan_walked(p)) {
    MpdataConvertJob b;
    b.j = wm_job(wm_plan(p), 0, nullptr, 0, p->ntracers);
    b.sel = block_sel(p, sl0, n);
    b.src = src; b.dst = dst;
    b.r = r; b.q0 = q0; b.y = y; b.limit = limit; b.dsum = dsum;
    HIP_TRY(mpdata_convert_wm(b, p->stream));
  } else {
    HIP_TRY(mpdata_convert_ref(p->f, p->eb, p->ncrms, sl0, n, p->nx, p->nz - 1, p->ntracers, src, dst, r, q0, y, limit, dsum, p->stream));
  }
  const int rc = plan_rewrote(p, sl0, n, src, 1, SEAMS | HALOS);
  return rc ? rc : plan_rewrote(p, sl0, n, dst, 1, SEAMS | HALOS);
}
// the pair, r and the mode of a call, for the plan forms (ntracers of the plan) and the array forms alike
static int convert_args(const char* what, int ntracers, int src, int dst, const void* r, int mode) {
  if (src < 0 || src >= ntracers || dst < 0 || dst >= ntracers)
    return set_err(MPDATA_EINVAL, "%s: tracer pair (src %d, dst %d) outside the %d tracers", what, src, dst, ntracers);
  if (src == dst) return set_err(MPDATA_EINVAL, "%s: src == dst (%d)", what, src);
  if (!r) return set_err(MPDATA_EINVAL, "%s: null r", what);
  if (mode & ~MPDATA_CONVERT_LIMIT) return set_err(MPDATA_EINVAL, "%s: unknown mode bits %d", what, mode);
  return 0;
}
static int plan_convert_check(const char* what, const mpdata_plan* p, int64_t sl0, int64_t n, int src, int dst, const void* r, int mode,
                              int eb) {
  int rc = block_range(what, p, sl0, n);
  if (rc) return rc;
  rc = convert_args(what, p->ntracers, src, dst, r, mode);
  return rc ? rc : plan_state(what, p, eb);
}
int mpdata_plan_convert_device(mpdata_plan* p, int64_t sl0, int64_t n, int src, int dst, const void* r, const void* q0, const void* y,
                               int mode, void* dsum) {
  const int rc = plan_convert_check("mpdata_plan_convert_device", p, sl0, n, src, dst, r, mode, 0);
  if (rc) return rc;
  DevGuard g(p->device);
  return plan_convert(p, sl0, n, src, dst, r, q0, y, mode, dsum);
}
static int plan_convert_host(mpdata_plan* p, int64_t sl0, int64_t n, int src, int dst, const void* r, const void* q0, const void* y,
                             int mode, void* dsum, int eb) {
  int rc = plan_convert_check("mpdata_plan_convert", p, sl0, n, src, dst, r, mode, eb);
  if (rc) return rc;
  DevGuard g(p->device);
  const size_t kb = (size_t)n * (p->nz - 1) * eb;
  HostArr a[4] = {{r, kb, false}, {q0, kb, false}, {y, kb, false}, {dsum, kb, true}};
  rc = stage_in(p, a);
  if (!rc) rc = plan_convert(p, sl0, n, src, dst, a[0].dev, a[1].dev, a[2].dev, mode, a[3].dev);
  return rc ? rc : stage_out(p, a);
}
int mpdata_plan_convert(mpdata_plan* p, int64_t sl0, int64_t n, int src, int dst, const double* r, const double* q0, const double* y,
                        int mode, double* dsum) {
  return plan_convert_host(p, sl0, n, src, dst, r, q0, y, mode, dsum, 8);
}
int mpdata_plan_convert_f32(mpdata_plan* p, int64_t sl0, int64_t n, int src, int dst, const float* r, const float* q0, const float* y,
                            int mode, float* dsum) {
  return plan_convert_host(p, sl0, n, src, dst, r, q0, y, mode, dsum, 4);
}
// the same on reference-layout device arrays (arguments checked before any device call): in place, asynchronous
static int convert_array(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, void* f, int src, int dst, const void* r,
                         const void* q0, const void* y, int mode, void* dsum, void* stream, int eb) {
  const char* const what = "mpdata_convert_device";
  int rc = array_sizes(what, ncrms, nx, nz, &ntracers);
  if (rc) return rc;
  rc = array_block(what, ncrms, sl0, n);
  if (rc) return rc;
  if (!f) return set_err(MPDATA_EINVAL, "%s: null f", what);
  rc = convert_args(what, ntracers, src, dst, r, mode);
  if (rc) return rc;
  HIP_TRY(mpdata_convert_ref(f, eb, ncrms, sl0, n, nx, nz - 1, ntracers, src, dst, r, q0, y, (mode & MPDATA_CONVERT_LIMIT) != 0, dsum,
                             (hipStream_t)stream));
  return 0;
}
int mpdata_convert_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, double* f, int src, int dst,
                          const double* r, const double* q0, const double* y, int mode, double* dsum, void* stream) {
  return convert_array(ncrms, nx, nz, ntracers, sl0, n, f, src, dst, r, q0, y, mode, dsum, stream, 8);
}
int mpdata_convert_f32_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, float* f, int src, int dst,
                              const float* r, const float* q0, const float* y, int mode, float* dsum, void* stream) {
  return convert_array(ncrms, nx, nz, ntracers, sl0, n, f, src, dst, r, q0, y, mode, dsum, stream, 4);
}

// ---- 3u: per-level covariance of two tracers of f: the sum over the interior columns of (a - m_a) * (b - m_b), m the given
// profile or the horizontal mean of the row, or of a * b (RAW).  Reads f, ma and mb, writes cov, mean_a and mean_b: as 3g,
// no flag of the plan is touched (the halo and seam marks stay -- halo columns are not read, owned levels are right
// whatever the seams hold), no event is recorded, and a windowed plan's inner plan is read where it lies.
static int plan_level_cov(mpdata_plan* p, int64_t sl0, int64_t n, int ta, int tb, const void* ma, const void* mb, int mode, void* cov,
                          void* mean_a, void* mean_b) {
  const int raw = (mode & MPDATA_LEVEL_COV_RAW) != 0;
  if (plan_walked(p)) {
    MpdataLevelCovJob b;
    b.j = wm_job(wm_plan(p), 0, nullptr, 0, p->ntracers);
    b.sel = block_sel(p, sl0, n);
    b.ta = ta; b.tb = tb;
    b.ma = ma; b.mb = mb; b.raw = raw; b.cov = cov; b.mean_a = mean_a; b.mean_b = mean_b;
    HIP_TRY(mpdata_level_cov_wm(b, p->stream));
  } else {
    HIP_TRY(mpdata_level_cov_ref(p->f, p->eb, p->ncrms, sl0, n, p->nx, p->nz - 1, p->ntracers, ta, tb, ma, mb, raw, cov, mean_a, mean_b,
                                 p->stream));
  }
  return 0;
}
// the pair, the mode and the arrays of a call, for the plan forms (ntracers of the plan) and the array forms alike
static int level_cov_args(const char* what, int ntracers, int ta, int tb, const void* ma, const void* mb, int mode, const void* cov,
                          const void* mean_a, const void* mean_b) {
  if (ta < 0 || ta >= ntracers || tb < 0 || tb >= ntracers)
    return set_err(MPDATA_EINVAL, "%s: tracer pair (ta %d, tb %d) outside the %d tracers", what, ta, tb, ntracers);
  if (mode & ~MPDATA_LEVEL_COV_RAW) return set_err(MPDATA_EINVAL, "%s: unknown mode bits %d", what, mode);
  if ((mode & MPDATA_LEVEL_COV_RAW) && (ma || mb || mean_a || mean_b))
    return set_err(MPDATA_EINVAL, "%s: MPDATA_LEVEL_COV_RAW with a non-null %s (RAW subtracts no mean)", what,
                   ma ? "ma" : mb ? "mb" : mean_a ? "mean_a" : "mean_b");
  if (!cov) return set_err(MPDATA_EINVAL, "%s: null cov", what);
  return 0;
}
static int plan_level_cov_check(const char* what, const mpdata_plan* p, int64_t sl0, int64_t n, int ta, int tb, const void* ma,
                                const void* mb, int mode, const void* cov, const void* mean_a, const void* mean_b, int eb) {
  int rc = block_range(what, p, sl0, n);
  if (rc) return rc;
  rc = level_cov_args(what, p->ntracers, ta, tb, ma, mb, mode, cov, mean_a, mean_b);
  return rc ? rc : plan_state(what, p, eb);
}
int mpdata_plan_level_cov_device(mpdata_plan* p, int64_t sl0, int64_t n, int ta, int tb, const void* ma, const void* mb, int mode,
                                 void* cov, void* mean_a, void* mean_b) {
  const int rc = plan_level_cov_check("mpdata_plan_level_cov_device", p, sl0, n, ta, tb, ma, mb, mode, cov, mean_a, mean_b, 0);
  if (rc) return rc;
  DevGuard g(p->device);
  return plan_level_cov(p, sl0, n, ta, tb, ma, mb, mode, cov, mean_a, mean_b);
}
static int plan_level_cov_host(mpdata_plan* p, int64_t sl0, int64_t n, int ta, int tb, const void* ma, const void* mb, int mode,
                               void* cov, void* mean_a, void* mean_b, int eb) {
  int rc = plan_level_cov_check("mpdata_plan_level_cov", p, sl0, n, ta, tb, ma, mb, mode, cov, mean_a, mean_b, eb);
  if (rc) return rc;
  DevGuard g(p->device);
  const size_t kb = (size_t)n * (p->nz - 1) * eb;
  HostArr a[5] = {{ma, kb, false}, {mb, kb, false}, {cov, kb, true}, {mean_a, kb, true}, {mean_b, kb, true}};
  rc = stage_in(p, a);
  if (!rc) rc = plan_level_cov(p, sl0, n, ta, tb, a[0].dev, a[1].dev, mode, a[2].dev, a[3].dev, a[4].dev);
  return rc ? rc : stage_out(p, a);
}
int mpdata_plan_level_cov(mpdata_plan* p, int64_t sl0, int64_t n, int ta, int tb, const double* ma, const double* mb, int mode,
                          double* cov, double* mean_a, double* mean_b) {
  return plan_level_cov_host(p, sl0, n, ta, tb, ma, mb, mode, cov, mean_a, mean_b, 8);
}
int mpdata_plan_level_cov_f32(mpdata_plan* p, int64_t sl0, int64_t n, int ta, int tb, const float* ma, const float* mb, int mode,
                              float* cov, float* mean_a, float* mean_b) {
  return plan_level_cov_host(p, sl0, n, ta, tb, ma, mb, mode, cov, mean_a, mean_b, 4);
}
// the same on reference-layout device arrays (arguments checked before any device call): asynchronous
static int level_cov_array(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, const void* f, int ta, int tb,
                           const void* ma, const void* mb, int mode, void* cov, void* mean_a, void* mean_b, void* stream, int eb) {
  const char* const what = "mpdata_level_cov_device";
  int rc = array_sizes(what, ncrms, nx, nz, &ntracers);
  if (rc) return rc;
  rc = array_block(what, ncrms, sl0, n);
  if (rc) return rc;
  if (!f) return set_err(MPDATA_EINVAL, "%s: null f", what);
  rc = level_cov_args(what, ntracers, ta, tb, ma, mb, mode, cov, mean_a, mean_b);
  if (rc) return rc;
  HIP_TRY(mpdata_level_cov_ref(f, eb, ncrms, sl0, n, nx, nz - 1, ntracers, ta, tb, ma, mb, (mode & MPDATA_LEVEL_COV_RAW) != 0, cov, mean_a,
                               mean_b, (hipStream_t)stream));
  return 0;
}
int mpdata_level_cov_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, const double* f, int ta, int tb,
                            const double* ma, const double* mb, int mode, double* cov, double* mean_a, double* mean_b, void* stream) {
  return level_cov_array(ncrms, nx, nz, ntracers, sl0, n, f, ta, tb, ma, mb, mode, cov, mean_a, mean_b, stream, 8);
}
int mpdata_level_cov_f32_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, const float* f, int ta, int tb,
                                const float* ma, const float* mb, int mode, float* cov, float* mean_a, float* mean_b, void* stream) {
  return level_cov_array(ncrms, nx, nz, ntracers, sl0, n, f, ta, tb, ma, mb, mode, cov, mean_a, mean_b, stream, 4);
}

// ---- 3v: per-level conditional counts and sums of f: how many interior columns have tracer tc inside (lo, hi], and the
// sum of every value tracer over exactly those columns.  Reads f, lo and hi, writes cnt and csum: as 3g and 3u, no flag of
// the plan is touched (the halo and seam marks stay -- halo columns are not read, owned levels are right whatever the
// seams hold), no event is recorded, and a windowed plan's inner plan is read where it lies.
static int plan_level_cond(mpdata_plan* p, int64_t sl0, int64_t n, int tc, const void* lo, const void* hi, void* cnt, void* csum,
                           int first, int count) {
  if (plan_walked(p)) {
    MpdataLevelCondJob b;
    b.j = wm_job(wm_plan(p), 0, nullptr, 0, p->ntracers);
    b.sel = block_sel(p, sl0, n);
    b.tc = tc; b.first = first; b.ntr = count;
    b.lo = lo; b.hi = hi; b.cnt = cnt; b.csum = csum;
    HIP_TRY(mpdata_level_cond_wm(b, p->stream));
  } else {
    HIP_TRY(mpdata_level_cond_ref(p->f, p->eb, p->ncrms, sl0, n, p->nx, p->nz - 1, p->ntracers, tc, lo, hi, cnt, csum, first, count,
                                  p->stream));
  }
  return 0;
}
// the condition, the bounds, the outputs and the value tracers of a call, for the plan forms (ntracers of the plan) and
// the array forms alike; without csum the range is not looked at
static int level_cond_args(const char* what, int ntracers, int tc, const void* lo, const void* hi, const void* cnt, const void* csum,
                           int first, int count) {
  if (tc < 0 || tc >= ntracers) return set_err(MPDATA_EINVAL, "%s: condition tracer tc %d outside the %d tracers", what, tc, ntracers);
  if (!lo && !hi) return set_err(MPDATA_EINVAL, "%s: lo and hi are both NULL", what);
  if (!cnt && !csum) return set_err(MPDATA_EINVAL, "%s: cnt and csum are both NULL", what);
  if (csum && (first < 0 || count < 1 || first > ntracers - count))
    return set_err(MPDATA_EINVAL, "%s: tracer range [%d, %lld) outside the %d tracers", what, first, (long long)first + count, ntracers);
  return 0;
}
static int plan_level_cond_check(const char* what, const mpdata_plan* p, int64_t sl0, int64_t n, int tc, const void* lo, const void* hi,
                                 const void* cnt, const void* csum, int first, int count, int eb) {
  int rc = block_range(what, p, sl0, n);
  if (rc) return rc;
  rc = level_cond_args(what, p->ntracers, tc, lo, hi, cnt, csum, first, count);
  return rc ? rc : plan_state(what, p, eb);
}
int mpdata_plan_level_cond_device(mpdata_plan* p, int64_t sl0, int64_t n, int tc, const void* lo, const void* hi, void* cnt, void* csum,
                                  int first_tracer, int ntracers) {
  const int rc = plan_level_cond_check("mpdata_plan_level_cond_device", p, sl0, n, tc, lo, hi, cnt, csum, first_tracer, ntracers, 0);
  if (rc) return rc;
  DevGuard g(p->device);
  return plan_level_cond(p, sl0, n, tc, lo, hi, cnt, csum, first_tracer, ntracers);
}
static int plan_level_cond_host(mpdata_plan* p, int64_t sl0, int64_t n, int tc, const void* lo, const void* hi, void* cnt, void* csum,
                                int eb) {
  int rc = plan_level_cond_check("mpdata_plan_level_cond", p, sl0, n, tc, lo, hi, cnt, csum, 0, p ? p->ntracers : 0, eb);
  if (rc) return rc;
  DevGuard g(p->device);
  const size_t kb = (size_t)n * (p->nz - 1) * eb;
  HostArr a[4] = {{lo, kb, false}, {hi, kb, false}, {cnt, kb, true}, {csum, kb * p->ntracers, true}};
  rc = stage_in(p, a);
  if (!rc) rc = plan_level_cond(p, sl0, n, tc, a[0].dev, a[1].dev, a[2].dev, a[3].dev, 0, p->ntracers);
  return rc ? rc : stage_out(p, a);
}
int mpdata_plan_level_cond(mpdata_plan* p, int64_t sl0, int64_t n, int tc, const double* lo, const double* hi, double* cnt, double* csum) {
  return plan_level_cond_host(p, sl0, n, tc, lo, hi, cnt, csum, 8);
}
int mpdata_plan_level_cond_f32(mpdata_plan* p, int64_t sl0, int64_t n, int tc, const float* lo, const float* hi, float* cnt, float* csum) {
  return plan_level_cond_host(p, sl0, n, tc, lo, hi, cnt, csum, 4);
}
// the same on reference-layout device arrays (arguments checked before any device call): asynchronous
static int level_cond_array(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, const void* f, int tc, const void* lo,
                            const void* hi, void* cnt, void* csum, int first, int count, void* stream, int eb) {
  const char* const what = "mpdata_level_cond_device";
  int rc = array_sizes(what, ncrms, nx, nz, &ntracers);
  if (rc) return rc;
  rc = array_block(what, ncrms, sl0, n);
  if (rc) return rc;
  if (!f) return set_err(MPDATA_EINVAL, "%s: null f", what);
  rc = level_cond_args(what, ntracers, tc, lo, hi, cnt, csum, first, count);
  if (rc) return rc;
  HIP_TRY(mpdata_level_cond_ref(f, eb, ncrms, sl0, n, nx, nz - 1, ntracers, tc, lo, hi, cnt, csum, first, count, (hipStream_t)stream));
  return 0;
}
int mpdata_level_cond_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, const double* f, int tc,
                             const double* lo, const double* hi, double* cnt, double* csum, int first_tracer, int ntr, void* stream) {
  return level_cond_array(ncrms, nx, nz, ntracers, sl0, n, f, tc, lo, hi, cnt, csum, first_tracer, ntr, stream, 8);
}
int mpdata_level_cond_f32_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, const float* f, int tc,
                                 const float* lo, const float* hi, float* cnt, float* csum, int first_tracer, int ntr, void* stream) {
  return level_cond_array(ncrms, nx, nz, ntracers, sl0, n, f, tc, lo, hi, cnt, csum, first_tracer, ntr, stream, 4);
}

// ---- 3w: per-column conditional level counts, bottoms, tops and paths of f: along the levels of every interior column,
// how many have tracer tc inside (lo, hi], the first and the last of them, and the mass-weighted integral of every value
// tracer over exactly those levels; cover and mass are their reductions over the columns.  Reads f, rho, adz, lo and hi,
// writes the outputs: as 3k and 3v, no flag of the plan is touched (the halo and seam marks stay -- halo columns are not
// read, owned levels are right whatever the seams hold), no event is recorded, a windowed plan's inner plan is read where
// it lies, and the velocities are not looked at.
struct ColumnCondOut {
  void *kcnt, *kbot, *ktop, *cpath, *cover, *mass;
};
static int plan_column_cond(mpdata_plan* p, int64_t sl0, int64_t n, int tc, const void* lo, const void* hi, const ColumnCondOut& o,
                            int first, int count) {
  if (!o.cpath) first = count = 0;
  if (plan_walked(p)) {
    const mpdata_plan* q = wm_plan(p);
    MpdataColumnCondJob b;
    b.j = wm_job(q, 0, nullptr, 0, p->ntracers);
    kc_rho_adz(q, b);
    b.sel = block_sel(p, sl0, n);
    b.tc = tc; b.first = first; b.ntr = count;
    b.lo = lo; b.hi = hi;
    b.kcnt = o.kcnt; b.kbot = o.kbot; b.ktop = o.ktop; b.cpath = o.cpath; b.cover = o.cover; b.mass = o.mass;
    HIP_TRY(mpdata_column_cond_wm(b, p->stream));
  } else {
    HIP_TRY(mpdata_column_cond_ref(p->f, p->rho, p->adz, p->eb, p->ncrms, sl0, n, p->nx, p->nz - 1, p->ntracers, tc, lo, hi, o.kcnt, o.kbot,
                                   o.ktop, o.cpath, o.cover, o.mass, first, count, p->stream));
  }
  return 0;
}
// the condition, the bounds, the outputs and the value tracers of a call, for the plan forms (ntracers of the plan) and
// the array forms alike; without cpath the range is not looked at
static int column_cond_args(const char* what, int ntracers, int tc, const void* lo, const void* hi, const ColumnCondOut& o, int first,
                            int count) {
  if (tc < 0 || tc >= ntracers) return set_err(MPDATA_EINVAL, "%s: condition tracer tc %d outside the %d tracers", what, tc, ntracers);
  if (!lo && !hi) return set_err(MPDATA_EINVAL, "%s: lo and hi are both NULL", what);
  if (!o.kcnt && !o.kbot && !o.ktop && !o.cpath && !o.cover && !o.mass) return set_err(MPDATA_EINVAL, "%s: every output is NULL", what);
  if (o.cover && !o.kcnt) return set_err(MPDATA_EINVAL, "%s: cover without kcnt", what);
  if (o.mass && !o.cpath) return set_err(MPDATA_EINVAL, "%s: mass without cpath", what);
  if (o.cpath && (first < 0 || count < 1 || first > ntracers - count))
    return set_err(MPDATA_EINVAL, "%s: tracer range [%d, %lld) outside the %d tracers", what, first, (long long)first + count, ntracers);
  return 0;
}
static int plan_column_cond_check(const char* what, const mpdata_plan* p, int64_t sl0, int64_t n, int tc, const void* lo, const void* hi,
                                  const ColumnCondOut& o, int first, int count, int eb) {
  int rc = block_range(what, p, sl0, n);
  if (rc) return rc;
  rc = column_cond_args(what, p->ntracers, tc, lo, hi, o, first, count);
  return rc ? rc : plan_state(what, p, eb);
}
int mpdata_plan_column_cond_device(mpdata_plan* p, int64_t sl0, int64_t n, int tc, const void* lo, const void* hi, void* kcnt, void* kbot,
                                   void* ktop, void* cpath, void* cover, void* mass, int first_tracer, int ntracers) {
  const ColumnCondOut o = {kcnt, kbot, ktop, cpath, cover, mass};
  const int rc = plan_column_cond_check("mpdata_plan_column_cond_device", p, sl0, n, tc, lo, hi, o, first_tracer, ntracers, 0);
  if (rc) return rc;
  DevGuard g(p->device);
  return plan_column_cond(p, sl0, n, tc, lo, hi, o, first_tracer, ntracers);
}
static int plan_column_cond_host(mpdata_plan* p, int64_t sl0, int64_t n, int tc, const void* lo, const void* hi, void* kcnt, void* kbot,
                                 void* ktop, void* cpath, void* cover, void* mass, int eb) {
  const ColumnCondOut o = {kcnt, kbot, ktop, cpath, cover, mass};
  int rc = plan_column_cond_check("mpdata_plan_column_cond", p, sl0, n, tc, lo, hi, o, 0, p ? p->ntracers : 0, eb);
  if (rc) return rc;
  DevGuard g(p->device);
  const size_t kb = (size_t)n * (p->nz - 1) * eb, xb = (size_t)n * p->nx * eb;
  HostArr a[8] = {{lo, kb, false}, {hi, kb, false}, {kcnt, xb, true}, {kbot, xb, true}, {ktop, xb, true}, {cpath, xb * p->ntracers, true},
                  {cover, (size_t)n * eb, true}, {mass, (size_t)n * p->ntracers * eb, true}};
  rc = stage_in(p, a);
  const ColumnCondOut d = {a[2].dev, a[3].dev, a[4].dev, a[5].dev, a[6].dev, a[7].dev};
  if (!rc) rc = plan_column_cond(p, sl0, n, tc, a[0].dev, a[1].dev, d, 0, p->ntracers);
  return rc ? rc : stage_out(p, a);
}
int mpdata_plan_column_cond(mpdata_plan* p, int64_t sl0, int64_t n, int tc, const double* lo, const double* hi, double* kcnt, double* kbot,
                            double* ktop, double* cpath, double* cover, double* mass) {
  return plan_column_cond_host(p, sl0, n, tc, lo, hi, kcnt, kbot, ktop, cpath, cover, mass, 8);
}
int mpdata_plan_column_cond_f32(mpdata_plan* p, int64_t sl0, int64_t n, int tc, const float* lo, const float* hi, float* kcnt, float* kbot,
                                float* ktop, float* cpath, float* cover, float* mass) {
  return plan_column_cond_host(p, sl0, n, tc, lo, hi, kcnt, kbot, ktop, cpath, cover, mass, 4);
}
// the same on reference-layout device arrays (arguments checked before any device call): asynchronous
static int column_cond_array(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, const void* f, const void* rho,
                             const void* adz, int tc, const void* lo, const void* hi, const ColumnCondOut& o, int first, int count,
                             void* stream, int eb) {
  const char* const what = "mpdata_column_cond_device";
  int rc = array_sizes(what, ncrms, nx, nz, &ntracers);
  if (rc) return rc;
  rc = array_block(what, ncrms, sl0, n);
  if (rc) return rc;
  if (!f || !rho || !adz) return set_err(MPDATA_EINVAL, "%s: null %s", what, !f ? "f" : !rho ? "rho" : "adz");
  rc = column_cond_args(what, ntracers, tc, lo, hi, o, first, count);
  if (rc) return rc;
  if (!o.cpath) first = count = 0;
  HIP_TRY(mpdata_column_cond_ref(f, rho, adz, eb, ncrms, sl0, n, nx, nz - 1, ntracers, tc, lo, hi, o.kcnt, o.kbot, o.ktop, o.cpath, o.cover,
                                 o.mass, first, count, (hipStream_t)stream));
  return 0;
}
int mpdata_column_cond_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, const double* f, const double* rho,
                              const double* adz, int tc, const double* lo, const double* hi, double* kcnt, double* kbot, double* ktop,
                              double* cpath, double* cover, double* mass, int first_tracer, int ntr, void* stream) {
  const ColumnCondOut o = {kcnt, kbot, ktop, cpath, cover, mass};
  return column_cond_array(ncrms, nx, nz, ntracers, sl0, n, f, rho, adz, tc, lo, hi, o, first_tracer, ntr, stream, 8);
}
int mpdata_column_cond_f32_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, const float* f, const float* rho,
                                  const float* adz, int tc, const float* lo, const float* hi, float* kcnt, float* kbot, float* ktop,
                                  float* cpath, float* cover, float* mass, int first_tracer, int ntr, void* stream) {
  const ColumnCondOut o = {kcnt, kbot, ktop, cpath, cover, mass};
  return column_cond_array(ncrms, nx, nz, ntracers, sl0, n, f, rho, adz, tc, lo, hi, o, first_tracer, ntr, stream, 4);
}

// ---- 3x: conservative per-level non-negativity fixer of f, in place: the negative cells of an interior row become +0 and
// the others are scaled so that the row keeps its sum; a row without a negative cell is read and not stored.  Writes sum
// and nneg, rewrites the INTERIOR columns of f of the block's instances and the tracer range; flux, u, w, rho, rhow, adz and
// the boundary mode are not touched and no event is recorded.  Halo marks, seam marks and the phantom: word for word as
// 3r's (plan_relax) -- the sums are over the owned level's own interior columns; the marks of the range are cleared
// whether a row was rewritten or not, since the host does not know.
static int plan_nonneg(mpdata_plan* p, int64_t sl0, int64_t n, void* sum, void* nneg, int first, int count) {
  if (plan_walked(p)) {
    MpdataNonnegJob b;
    b.j = wm_job(wm_plan(p), 0, nullptr, first, count);
    b.sel = block_sel(p, sl0, n);
    b.sum = sum; b.nneg = nneg;
    HIP_TRY(mpdata_nonneg_wm(b, p->stream));
  } else {
    HIP_TRY(mpdata_nonneg_ref(ref_f(p, first), p->eb, p->ncrms, sl0, n, p->nx, p->nz - 1, count, sum, nneg, p->stream));
  }
  return plan_rewrote(p, sl0, n, first, count, SEAMS | HALOS);
}
static int plan_nonneg_check(const char* what, const mpdata_plan* p, int64_t sl0, int64_t n, int first, int count, int eb) {
  const int rc = block_ranges(what, p, sl0, n, first, count, eb);
  return rc ? rc : plan_state(what, p, eb);
}
int mpdata_plan_nonneg_device(mpdata_plan* p, int64_t sl0, int64_t n, void* sum, void* nneg, int first_tracer, int ntracers) {
  const int rc = plan_nonneg_check("mpdata_plan_nonneg_device", p, sl0, n, first_tracer, ntracers, 0);
  if (rc) return rc;
  DevGuard g(p->device);
  return plan_nonneg(p, sl0, n, sum, nneg, first_tracer, ntracers);
}
static int plan_nonneg_host(mpdata_plan* p, int64_t sl0, int64_t n, void* sum, void* nneg, int eb) {
  int rc = plan_nonneg_check("mpdata_plan_nonneg", p, sl0, n, 0, 0, eb);
  if (rc) return rc;
  DevGuard g(p->device);
  const size_t kb = (size_t)n * (p->nz - 1) * eb * p->ntracers;
  HostArr a[2] = {{sum, kb, true}, {nneg, kb, true}};
  rc = stage_in(p, a);
  if (!rc) rc = plan_nonneg(p, sl0, n, a[0].dev, a[1].dev, 0, p->ntracers);
  return rc ? rc : stage_out(p, a);
}
int mpdata_plan_nonneg(mpdata_plan* p, int64_t sl0, int64_t n, double* sum, double* nneg) {
  return plan_nonneg_host(p, sl0, n, sum, nneg, 8);
}
int mpdata_plan_nonneg_f32(mpdata_plan* p, int64_t sl0, int64_t n, float* sum, float* nneg) {
  return plan_nonneg_host(p, sl0, n, sum, nneg, 4);
}
// the same on reference-layout device arrays (arguments checked before any device call): in place, asynchronous
static int nonneg_array(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, void* f, void* sum, void* nneg, void* stream,
                        int eb) {
  int rc = array_sizes("mpdata_nonneg_device", ncrms, nx, nz, &ntracers);
  if (rc) return rc;
  rc = array_block("mpdata_nonneg_device", ncrms, sl0, n);
  if (rc) return rc;
  if (!f) return set_err(MPDATA_EINVAL, "mpdata_nonneg_device: null f");
  HIP_TRY(mpdata_nonneg_ref(f, eb, ncrms, sl0, n, nx, nz - 1, ntracers, sum, nneg, (hipStream_t)stream));
  return 0;
}
int mpdata_nonneg_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, double* f, double* sum, double* nneg,
                         void* stream) {
  return nonneg_array(ncrms, nx, nz, ntracers, sl0, n, f, sum, nneg, stream, 8);
}
int mpdata_nonneg_f32_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, float* f, float* sum, float* nneg,
                             void* stream) {
  return nonneg_array(ncrms, nx, nz, ntracers, sl0, n, f, sum, nneg, stream, 4);
}

// ---- 3y: saturation adjustment of the tracers of f, in place: the condensate (tracer tn) and on request the temperature
// (tracer tt) from a temperature-like tracer th and total water tq, by a Newton iteration per cell on the caller's curves.
// Reads pres and gz, writes ncld and iters, reads the INTERIOR columns of th and tq and rewrites those of tn and tt of the
// block's instances; every other tracer, flux, u, w, rho, rhow, adz and the boundary mode are not touched and no event is
// recorded.  Halo marks, seam marks and the phantom of tn and tt: word for word as 3t's (plan_convert) for its two tracers;
// the marks of th and tq do not change.
static MpdataSatadjArgs satadj_args(int eb, int th, int tq, int tn, int tt, const void* pres, const void* gz,
                                    const mpdata_satadj_params* par, int mode, void* ncld, void* iters) {
  MpdataSatadjArgs a;
  a.th = th; a.tq = tq; a.tn = tn; a.tt = tt;
  a.pres = pres; a.gz = gz; a.ice = (mode & MPDATA_SATADJ_ICE) != 0; a.ncld = ncld; a.iters = iters;
  if (eb == 8) satadj_par(par, &a.par.d);
  else satadj_par(par, &a.par.f);
  return a;
}
static int plan_satadj(mpdata_plan* p, int64_t sl0, int64_t n, const MpdataSatadjArgs& a) {
  if (plan_walked(p)) {
    MpdataSatadjJob b;
    b.j = wm_job(wm_plan(p), 0, nullptr, 0, p->ntracers);
    b.sel = block_sel(p, sl0, n);
    b.a = a;
    HIP_TRY(mpdata_satadj_wm(b, p->stream));
  } else {
    HIP_TRY(mpdata_satadj_ref(p->f, p->eb, p->ncrms, sl0, n, p->nx, p->nz - 1, p->ntracers, a, p->stream));
  }
  const int rc = plan_rewrote(p, sl0, n, a.tn, 1, SEAMS | HALOS);
  return rc || a.tt < 0 ? rc : plan_rewrote(p, sl0, n, a.tt, 1, SEAMS | HALOS);
}
// the tracers, the rows, the numbers and the mode of a call, for the plan forms (ntracers of the plan) and the array forms alike
static int satadj_check(const char* what, int ntracers, int th, int tq, int tn, int tt, const void* pres, const mpdata_satadj_params* par,
                        int mode) {
  if (th < 0 || th >= ntracers || tq < 0 || tq >= ntracers || tn < 0 || tn >= ntracers)
    return set_err(MPDATA_EINVAL, "%s: tracers (th %d, tq %d, tn %d) outside the %d tracers", what, th, tq, tn, ntracers);
  if (tt < -1 || tt >= ntracers) return set_err(MPDATA_EINVAL, "%s: tt = %d outside [-1, %d)", what, tt, ntracers);
  if (th == tq || th == tn || tq == tn || tt == th || tt == tq || tt == tn)
    return set_err(MPDATA_EINVAL, "%s: tracers th %d, tq %d, tn %d, tt %d are not distinct", what, th, tq, tn, tt);
  if (!pres) return set_err(MPDATA_EINVAL, "%s: null pres", what);
  if (!par) return set_err(MPDATA_EINVAL, "%s: null par", what);
  if (par->maxit < 1 || par->maxit > 32) return set_err(MPDATA_EINVAL, "%s: maxit = %d outside 1 .. 32", what, par->maxit);
  if (!(par->tol >= 0)) return set_err(MPDATA_EINVAL, "%s: tol = %g is not >= 0", what, par->tol);
  if ((mode & MPDATA_SATADJ_ICE) && !(par->tmax > par->tmin))
    return set_err(MPDATA_EINVAL, "%s: tmax = %g is not > tmin = %g", what, par->tmax, par->tmin);
  if (mode & ~MPDATA_SATADJ_ICE) return set_err(MPDATA_EINVAL, "%s: unknown mode bits %d", what, mode);
  return 0;
}
static int plan_satadj_check(const char* what, const mpdata_plan* p, int64_t sl0, int64_t n, int th, int tq, int tn, int tt,
                             const void* pres, const mpdata_satadj_params* par, int mode, int eb) {
  int rc = block_range(what, p, sl0, n);
  if (rc) return rc;
  rc = satadj_check(what, p->ntracers, th, tq, tn, tt, pres, par, mode);
  return rc ? rc : plan_state(what, p, eb);
}
int mpdata_plan_satadj_device(mpdata_plan* p, int64_t sl0, int64_t n, int th, int tq, int tn, int tt, const void* pres, const void* gz,
                              const mpdata_satadj_params* par, int mode, void* ncld, void* iters) {
  const int rc = plan_satadj_check("mpdata_plan_satadj_device", p, sl0, n, th, tq, tn, tt, pres, par, mode, 0);
  if (rc) return rc;
  DevGuard g(p->device);
  return plan_satadj(p, sl0, n, satadj_args(p->eb, th, tq, tn, tt, pres, gz, par, mode, ncld, iters));
}
static int plan_satadj_host(mpdata_plan* p, int64_t sl0, int64_t n, int th, int tq, int tn, int tt, const void* pres, const void* gz,
                            const mpdata_satadj_params* par, int mode, void* ncld, void* iters, int eb) {
  int rc = plan_satadj_check("mpdata_plan_satadj", p, sl0, n, th, tq, tn, tt, pres, par, mode, eb);
  if (rc) return rc;
  DevGuard g(p->device);
  const size_t kb = (size_t)n * (p->nz - 1) * eb;
  HostArr a[4] = {{pres, kb, false}, {gz, kb, false}, {ncld, kb, true}, {iters, kb, true}};
  rc = stage_in(p, a);
  if (!rc) rc = plan_satadj(p, sl0, n, satadj_args(eb, th, tq, tn, tt, a[0].dev, a[1].dev, par, mode, a[2].dev, a[3].dev));
  return rc ? rc : stage_out(p, a);
}
int mpdata_plan_satadj(mpdata_plan* p, int64_t sl0, int64_t n, int th, int tq, int tn, int tt, const double* pres, const double* gz,
                       const mpdata_satadj_params* par, int mode, double* ncld, double* iters) {
  return plan_satadj_host(p, sl0, n, th, tq, tn, tt, pres, gz, par, mode, ncld, iters, 8);
}
int mpdata_plan_satadj_f32(mpdata_plan* p, int64_t sl0, int64_t n, int th, int tq, int tn, int tt, const float* pres, const float* gz,
                           const mpdata_satadj_params* par, int mode, float* ncld, float* iters) {
  return plan_satadj_host(p, sl0, n, th, tq, tn, tt, pres, gz, par, mode, ncld, iters, 4);
}
// the same on reference-layout device arrays (arguments checked before any device call): in place, asynchronous
static int satadj_array(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, void* f, int th, int tq, int tn, int tt,
                        const void* pres, const void* gz, const mpdata_satadj_params* par, int mode, void* ncld, void* iters, void* stream,
                        int eb) {
  const char* const what = "mpdata_satadj_device";
  int rc = array_sizes(what, ncrms, nx, nz, &ntracers);
  if (rc) return rc;
  rc = array_block(what, ncrms, sl0, n);
  if (rc) return rc;
  if (!f) return set_err(MPDATA_EINVAL, "%s: null f", what);
  rc = satadj_check(what, ntracers, th, tq, tn, tt, pres, par, mode);
  if (rc) return rc;
  HIP_TRY(mpdata_satadj_ref(f, eb, ncrms, sl0, n, nx, nz - 1, ntracers, satadj_args(eb, th, tq, tn, tt, pres, gz, par, mode, ncld, iters),
                            (hipStream_t)stream));
  return 0;
}
int mpdata_satadj_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, double* f, int th, int tq, int tn, int tt,
                         const double* pres, const double* gz, const mpdata_satadj_params* par, int mode, double* ncld, double* iters,
                         void* stream) {
  return satadj_array(ncrms, nx, nz, ntracers, sl0, n, f, th, tq, tn, tt, pres, gz, par, mode, ncld, iters, stream, 8);
}
int mpdata_satadj_f32_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, float* f, int th, int tq, int tn, int tt,
                             const float* pres, const float* gz, const mpdata_satadj_params* par, int mode, float* ncld, float* iters,
                             void* stream) {
  return satadj_array(ncrms, nx, nz, ntracers, sl0, n, f, th, tq, tn, tt, pres, gz, par, mode, ncld, iters, stream, 4);
}

// ---- 3z: linear combination of tracers of f, in place: f(dst) = sum over j of coef_j * f(src_j) + c0 on the interior
// columns, clipped at zero on request.  Reads coef and c0 and the sources, writes sum, rewrites the INTERIOR columns of
// tracer dst of the block's instances; every other tracer (the sources that are not dst among them), flux, u, w, rho, rhow,
// adz and the boundary mode are not touched and no event is recorded.  Halo marks, seam marks and the phantom: word for
// word as 3t's (plan_convert), for the ONE written tracer dst; the marks of the sources are not touched -- the call reads
// their interior columns and owned levels only, which are right whatever their halos and seams hold.
static int plan_combine(mpdata_plan* p, int64_t sl0, int64_t n, int dst, int nsrc, const int* src, const void* coef, const void* c0,
                        int mode, void* sum) {
  const int clip = (mode & MPDATA_COMBINE_CLIP) != 0;
  if (plan_walked(p)) {
    MpdataCombineJob b;
    b.j = wm_job(wm_plan(p), 0, nullptr, 0, p->ntracers);
    b.sel = block_sel(p, sl0, n);
    b.dst = dst; b.nsrc = nsrc;
    for (int q = 0; q < MPDATA_COMBINE_MAX; ++q) { b.src[q] = q < nsrc ? src[q] : dst; b.off[q] = 0; }
    b.coef = coef; b.c0 = c0; b.clip = clip; b.sum = sum;
    HIP_TRY(mpdata_combine_wm(b, p->stream));
  } else {
    HIP_TRY(mpdata_combine_ref(p->f, p->eb, p->ncrms, sl0, n, p->nx, p->nz - 1, p->ntracers, dst, nsrc, src, coef, c0, clip, sum, p->stream));
  }
  return plan_rewrote(p, sl0, n, dst, 1, SEAMS | HALOS);
}
// dst, the sources, c0 and the mode of a call, for the plan forms (ntracers of the plan) and the array forms alike
static int combine_args(const char* what, int ntracers, int dst, int nsrc, const int* src, const void* c0, int mode) {
  if (dst < 0 || dst >= ntracers) return set_err(MPDATA_EINVAL, "%s: dst %d outside the %d tracers", what, dst, ntracers);
  if (nsrc < 0 || nsrc > MPDATA_COMBINE_MAX) return set_err(MPDATA_EINVAL, "%s: nsrc %d outside [0, %d]", what, nsrc, MPDATA_COMBINE_MAX);
  if (nsrc > 0 && !src) return set_err(MPDATA_EINVAL, "%s: null src", what);
  for (int j = 0; j < nsrc; ++j)
    if (src[j] < 0 || src[j] >= ntracers)
      return set_err(MPDATA_EINVAL, "%s: source %d (src[%d]) outside the %d tracers", what, src[j], j, ntracers);
  if (nsrc == 0 && !c0) return set_err(MPDATA_EINVAL, "%s: null c0 with nsrc == 0", what);
  if (mode & ~MPDATA_COMBINE_CLIP) return set_err(MPDATA_EINVAL, "%s: unknown mode bits %d", what, mode);
  return 0;
}
static int plan_combine_check(const char* what, const mpdata_plan* p, int64_t sl0, int64_t n, int dst, int nsrc, const int* src,
                              const void* c0, int mode, int eb) {
  int rc = block_range(what, p, sl0, n);
  if (rc) return rc;
  rc = combine_args(what, p->ntracers, dst, nsrc, src, c0, mode);
  return rc ? rc : plan_state(what, p, eb);
}
int mpdata_plan_combine_device(mpdata_plan* p, int64_t sl0, int64_t n, int dst, int nsrc, const int* src, const void* coef,
                               const void* c0, int mode, void* sum) {
  const int rc = plan_combine_check("mpdata_plan_combine_device", p, sl0, n, dst, nsrc, src, c0, mode, 0);
  if (rc) return rc;
  DevGuard g(p->device);
  return plan_combine(p, sl0, n, dst, nsrc, src, coef, c0, mode, sum);
}
static int plan_combine_host(mpdata_plan* p, int64_t sl0, int64_t n, int dst, int nsrc, const int* src, const void* coef, const void* c0,
                             int mode, void* sum, int eb) {
  int rc = plan_combine_check("mpdata_plan_combine", p, sl0, n, dst, nsrc, src, c0, mode, eb);
  if (rc) return rc;
  DevGuard g(p->device);
  const size_t kb = (size_t)n * (p->nz - 1) * eb;
  HostArr a[3] = {{nsrc > 0 ? coef : nullptr, kb * nsrc, false}, {c0, kb, false}, {sum, kb, true}};
  rc = stage_in(p, a);
  if (!rc) rc = plan_combine(p, sl0, n, dst, nsrc, src, a[0].dev, a[1].dev, mode, a[2].dev);
  return rc ? rc : stage_out(p, a);
}
int mpdata_plan_combine(mpdata_plan* p, int64_t sl0, int64_t n, int dst, int nsrc, const int* src, const double* coef, const double* c0,
                        int mode, double* sum) {
  return plan_combine_host(p, sl0, n, dst, nsrc, src, coef, c0, mode, sum, 8);
}
int mpdata_plan_combine_f32(mpdata_plan* p, int64_t sl0, int64_t n, int dst, int nsrc, const int* src, const float* coef,
                            const float* c0, int mode, float* sum) {
  return plan_combine_host(p, sl0, n, dst, nsrc, src, coef, c0, mode, sum, 4);
}
// the same on reference-layout device arrays (arguments checked before any device call): in place, asynchronous
static int combine_array(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, void* f, int dst, int nsrc, const int* src,
                         const void* coef, const void* c0, int mode, void* sum, void* stream, int eb) {
  const char* const what = "mpdata_combine_device";
  int rc = array_sizes(what, ncrms, nx, nz, &ntracers);
  if (rc) return rc;
  rc = array_block(what, ncrms, sl0, n);
  if (rc) return rc;
  if (!f) return set_err(MPDATA_EINVAL, "%s: null f", what);
  rc = combine_args(what, ntracers, dst, nsrc, src, c0, mode);
  if (rc) return rc;
  HIP_TRY(mpdata_combine_ref(f, eb, ncrms, sl0, n, nx, nz - 1, ntracers, dst, nsrc, src, coef, c0, (mode & MPDATA_COMBINE_CLIP) != 0, sum,
                             (hipStream_t)stream));
  return 0;
}
int mpdata_combine_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, double* f, int dst, int nsrc,
                          const int* src, const double* coef, const double* c0, int mode, double* sum, void* stream) {
  return combine_array(ncrms, nx, nz, ntracers, sl0, n, f, dst, nsrc, src, coef, c0, mode, sum, stream, 8);
}
int mpdata_combine_f32_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, float* f, int dst, int nsrc,
                              const int* src, const float* coef, const float* c0, int mode, float* sum, void* stream) {
  return combine_array(ncrms, nx, nz, ntracers, sl0, n, f, dst, nsrc, src, coef, c0, mode, sum, stream, 4);
}

// ---- 3aa: running column integral of tracer src into tracer dst, in place: o(k) = the sum of wgt * f(src) from the surface
// up to k (or from the top down to it), f(dst) = o on the interior columns, total = the final sum per column.  Reads wgt (or
// the plan's rho and adz) and the interior of src, writes total, rewrites the INTERIOR columns of tracer dst of the block's
// instances; every other tracer (src where it is not dst among them), flux, u, w, rho, rhow, adz and the boundary mode are
// not touched and no event is recorded.  Halo marks, seam marks and the phantom: word for word as 3z's (plan_combine), for
// the ONE written tracer dst; the marks of src are not touched -- the call reads its interior columns and owned levels
// only, which are right whatever its halos and seams hold.  The velocities are not looked at.
static int plan_column_scan(mpdata_plan* p, int64_t sl0, int64_t n, int src, int dst, const void* wgt, void* total, int mode) {
  if (plan_walked(p)) {
    const mpdata_plan* q = wm_plan(p);
    MpdataColumnScanJob b;
    b.j = wm_job(q, 0, nullptr, src, 1);
    kc_rho_adz(q, b);
    b.sel = block_sel(p, sl0, n);
    b.doff = (long long)(dst - src) * b.j.prv_tstride;
    b.wgt = wgt; b.total = total; b.mode = mode;
    HIP_TRY(mpdata_column_scan_wm(b, p->stream));
  } else {
    HIP_TRY(mpdata_column_scan_ref(p->f, p->eb, p->ncrms, sl0, n, p->nx, p->nz - 1, p->ntracers, src, dst, wgt, p->rho, p->adz, total, mode,
                                   p->stream));
  }
  return plan_rewrote(p, sl0, n, dst, 1, SEAMS | HALOS);
}
// src, dst and the mode of a call, for the plan forms (ntracers of the plan) and the array forms alike
static int column_scan_args(const char* what, int ntracers, int src, int dst, int mode) {
  if (src < 0 || src >= ntracers) return set_err(MPDATA_EINVAL, "%s: src %d outside the %d tracers", what, src, ntracers);
  if (dst < 0 || dst >= ntracers) return set_err(MPDATA_EINVAL, "%s: dst %d outside the %d tracers", what, dst, ntracers);
  if (mode & ~(MPDATA_COLUMN_SCAN_DOWN | MPDATA_COLUMN_SCAN_EXCLUSIVE)) return set_err(MPDATA_EINVAL, "%s: unknown mode bits %d", what, mode);
  return 0;
}
static int plan_column_scan_check(const char* what, const mpdata_plan* p, int64_t sl0, int64_t n, int src, int dst, int mode, int eb) {
  int rc = block_range(what, p, sl0, n);
  if (rc) return rc;
  rc = column_scan_args(what, p->ntracers, src, dst, mode);
  return rc ? rc : plan_state(what, p, eb);
}
int mpdata_plan_column_scan_device(mpdata_plan* p, int64_t sl0, int64_t n, int src, int dst, const void* wgt, void* total, int mode) {
  const int rc = plan_column_scan_check("mpdata_plan_column_scan_device", p, sl0, n, src, dst, mode, 0);
  if (rc) return rc;
  DevGuard g(p->device);
  return plan_column_scan(p, sl0, n, src, dst, wgt, total, mode);
}
static int plan_column_scan_host(mpdata_plan* p, int64_t sl0, int64_t n, int src, int dst, const void* wgt, void* total, int mode, int eb) {
  int rc = plan_column_scan_check("mpdata_plan_column_scan", p, sl0, n, src, dst, mode, eb);
  if (rc) return rc;
  DevGuard g(p->device);
  HostArr a[2] = {{wgt, (size_t)n * (p->nz - 1) * eb, false}, {total, (size_t)n * p->nx * eb, true}};
  rc = stage_in(p, a);
  if (!rc) rc = plan_column_scan(p, sl0, n, src, dst, a[0].dev, a[1].dev, mode);
  return rc ? rc : stage_out(p, a);
}
int mpdata_plan_column_scan(mpdata_plan* p, int64_t sl0, int64_t n, int src, int dst, const double* wgt, double* total, int mode) {
  return plan_column_scan_host(p, sl0, n, src, dst, wgt, total, mode, 8);
}
int mpdata_plan_column_scan_f32(mpdata_plan* p, int64_t sl0, int64_t n, int src, int dst, const float* wgt, float* total, int mode) {
  return plan_column_scan_host(p, sl0, n, src, dst, wgt, total, mode, 4);
}
// the same on reference-layout device arrays (arguments checked before any device call): in place, asynchronous; wgt is
// required -- the arrays have no rho and adz
static int column_scan_array(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, void* f, int src, int dst, const void* wgt,
                             void* total, int mode, void* stream, int eb) {
  const char* const what = "mpdata_column_scan_device";
  int rc = array_sizes(what, ncrms, nx, nz, &ntracers);
  if (rc) return rc;
  rc = array_block(what, ncrms, sl0, n);
  if (rc) return rc;
  if (!f) return set_err(MPDATA_EINVAL, "%s: null f", what);
  if (!wgt) return set_err(MPDATA_EINVAL, "%s: null wgt", what);
  rc = column_scan_args(what, ntracers, src, dst, mode);
  if (rc) return rc;
  HIP_TRY(mpdata_column_scan_ref(f, eb, ncrms, sl0, n, nx, nz - 1, ntracers, src, dst, wgt, nullptr, nullptr, total, mode, (hipStream_t)stream));
  return 0;
}
int mpdata_column_scan_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, double* f, int src, int dst,
                              const double* wgt, double* total, int mode, void* stream) {
  return column_scan_array(ncrms, nx, nz, ntracers, sl0, n, f, src, dst, wgt, total, mode, stream, 8);
}
int mpdata_column_scan_f32_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, float* f, int src, int dst,
                                  const float* wgt, float* total, int mode, void* stream) {
  return column_scan_array(ncrms, nx, nz, ntracers, sl0, n, f, src, dst, wgt, total, mode, stream, 4);
}

// ---- 3ab: per-level histograms of f: how many interior columns have tracer tc inside each of the nb bins (e_j, e_{j+1}],
// and the sum of every value tracer over exactly the columns of each bin.  Reads f and the HOST array edges, writes cnt and
// bsum: as 3v, no flag of the plan is touched, no event is recorded, and a windowed plan's inner plan is read where it lies.
static int plan_level_hist(mpdata_plan* p, int64_t sl0, int64_t n, int tc, int nb, const double* edges, void* cnt, void* bsum, int first,
                           int count) {
  if (plan_walked(p)) {
    MpdataLevelHistJob b;
    b.j = wm_job(wm_plan(p), 0, nullptr, 0, p->ntracers);
    b.sel = block_sel(p, sl0, n);
    b.tc = tc; b.first = first; b.ntr = count; b.nb = nb;
    b.cnt = cnt; b.bsum = bsum;
    HIP_TRY(mpdata_level_hist_wm(b, edges, p->stream));
  } else {
    HIP_TRY(mpdata_level_hist_ref(p->f, p->eb, p->ncrms, sl0, n, p->nx, p->nz - 1, p->ntracers, tc, nb, edges, cnt, bsum, first, count,
                                  p->stream));
  }
  return 0;
}
// the binned tracer, the bins, the outputs and the value tracers of a call, for the plan forms (ntracers of the plan) and
// the array forms alike; the edges are checked as given (rounding to fp32 is monotone); without bsum the range is not
// looked at
static int level_hist_args(const char* what, int ntracers, int tc, int nb, const double* edges, const void* cnt, const void* bsum,
                           int first, int count) {
  if (tc < 0 || tc >= ntracers) return set_err(MPDATA_EINVAL, "%s: binned tracer tc %d outside the %d tracers", what, tc, ntracers);
  if (nb < 1 || nb > MPDATA_LEVEL_HIST_MAX_BINS)
    return set_err(MPDATA_EINVAL, "%s: nb %d outside [1, %d]", what, nb, MPDATA_LEVEL_HIST_MAX_BINS);
  if (!edges) return set_err(MPDATA_EINVAL, "%s: null edges", what);
  for (int j = 0; j <= nb; ++j) {
    if (edges[j] != edges[j]) return set_err(MPDATA_EINVAL, "%s: edges[%d] is a NaN", what, j);
    if (j < nb && edges[j] > edges[j + 1]) return set_err(MPDATA_EINVAL, "%s: edges[%d] > edges[%d]", what, j, j + 1);
  }
  if (!cnt && !bsum) return set_err(MPDATA_EINVAL, "%s: cnt and bsum are both NULL", what);
  if (bsum && (first < 0 || count < 1 || first > ntracers - count))
    return set_err(MPDATA_EINVAL, "%s: tracer range [%d, %lld) outside the %d tracers", what, first, (long long)first + count, ntracers);
  return 0;
}
static int plan_level_hist_check(const char* what, const mpdata_plan* p, int64_t sl0, int64_t n, int tc, int nb, const double* edges,
                                 const void* cnt, const void* bsum, int first, int count, int eb) {
  int rc = block_range(what, p, sl0, n);
  if (rc) return rc;
  rc = level_hist_args(what, p->ntracers, tc, nb, edges, cnt, bsum, first, count);
  return rc ? rc : plan_state(what, p, eb);
}
int mpdata_plan_level_hist_device(mpdata_plan* p, int64_t sl0, int64_t n, int tc, int nb, const double* edges, void* cnt, void* bsum,
                                  int first_tracer, int ntracers) {
  const int rc = plan_level_hist_check("mpdata_plan_level_hist_device", p, sl0, n, tc, nb, edges, cnt, bsum, first_tracer, ntracers, 0);
  if (rc) return rc;
  DevGuard g(p->device);
  return plan_level_hist(p, sl0, n, tc, nb, edges, cnt, bsum, first_tracer, ntracers);
}
static int plan_level_hist_host(mpdata_plan* p, int64_t sl0, int64_t n, int tc, int nb, const double* edges, void* cnt, void* bsum, int eb) {
  int rc = plan_level_hist_check("mpdata_plan_level_hist", p, sl0, n, tc, nb, edges, cnt, bsum, 0, p ? p->ntracers : 0, eb);
  if (rc) return rc;
  DevGuard g(p->device);
  const size_t kb = (size_t)n * (p->nz - 1) * nb * eb;
  HostArr a[2] = {{cnt, kb, true}, {bsum, kb * p->ntracers, true}};
  rc = stage_in(p, a);
  if (!rc) rc = plan_level_hist(p, sl0, n, tc, nb, edges, a[0].dev, a[1].dev, 0, p->ntracers);
  return rc ? rc : stage_out(p, a);
}
int mpdata_plan_level_hist(mpdata_plan* p, int64_t sl0, int64_t n, int tc, int nb, const double* edges, double* cnt, double* bsum) {
  return plan_level_hist_host(p, sl0, n, tc, nb, edges, cnt, bsum, 8);
}
int mpdata_plan_level_hist_f32(mpdata_plan* p, int64_t sl0, int64_t n, int tc, int nb, const double* edges, float* cnt, float* bsum) {
  return plan_level_hist_host(p, sl0, n, tc, nb, edges, cnt, bsum, 4);
}
// the same on reference-layout device arrays (arguments checked before any device call): asynchronous
static int level_hist_array(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, const void* f, int tc, int nb,
                            const double* edges, void* cnt, void* bsum, int first, int count, void* stream, int eb) {
  const char* const what = "mpdata_level_hist_device";
  int rc = array_sizes(what, ncrms, nx, nz, &ntracers);
  if (rc) return rc;
  rc = array_block(what, ncrms, sl0, n);
  if (rc) return rc;
  if (!f) return set_err(MPDATA_EINVAL, "%s: null f", what);
  rc = level_hist_args(what, ntracers, tc, nb, edges, cnt, bsum, first, count);
  if (rc) return rc;
  HIP_TRY(mpdata_level_hist_ref(f, eb, ncrms, sl0, n, nx, nz - 1, ntracers, tc, nb, edges, cnt, bsum, first, count, (hipStream_t)stream));
  return 0;
}
int mpdata_level_hist_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, const double* f, int tc, int nb,
                             const double* edges, double* cnt, double* bsum, int first_tracer, int ntr, void* stream) {
  return level_hist_array(ncrms, nx, nz, ntracers, sl0, n, f, tc, nb, edges, cnt, bsum, first_tracer, ntr, stream, 8);
}
int mpdata_level_hist_f32_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, const float* f, int tc, int nb,
                                 const double* edges, float* cnt, float* bsum, int first_tracer, int ntr, void* stream) {
  return level_hist_array(ncrms, nx, nz, ntracers, sl0, n, f, tc, nb, edges, cnt, bsum, first_tracer, ntr, stream, 4);
}

// ---- 3ac: per-level updraft / downdraft sampling of f by the cell-centred w: the interior columns of a level in three
// classes by wc = 0.5 * (w(k) + w(k+1)) against wup and wdn, where tracer tc lies inside (lo, hi]; per class the count, the
// sum of wc, of every value tracer and of wc * tracer.  Reads f, w, lo and hi, writes the four outputs: as 3h and 3v, no
// flag of the plan is touched, no event is recorded, and a windowed plan's inner plan is read where it lies.  The plan must
// hold w; u is not looked at.
struct LevelDraftOut {
  void *cnt, *wsum, *fsum, *wfsum;
};
static int plan_level_draft(mpdata_plan* p, int64_t sl0, int64_t n, int tc, const void* lo, const void* hi, double wup, double wdn,
                            const LevelDraftOut& o, int first, int count) {
  if (plan_walked(p)) {
    const mpdata_plan* q = wm_plan(p);
    MpdataLevelDraftJob b;
    b.j = wm_job(q, 0, nullptr, 0, p->ntracers);
    b.w = wm_job(q, 2, nullptr, 0, 1).prv;
    b.sel = block_sel(p, sl0, n);
    b.tc = tc; b.first = first; b.ntr = count;
    b.lo = lo; b.hi = hi; b.wup = wup; b.wdn = wdn;
    b.cnt = o.cnt; b.wsum = o.wsum; b.fsum = o.fsum; b.wfsum = o.wfsum;
    HIP_TRY(mpdata_level_draft_wm(b, p->stream));
  } else {
    HIP_TRY(mpdata_level_draft_ref(p->f, p->w, p->eb, p->ncrms, sl0, n, p->nx, p->nz - 1, p->ntracers, tc, lo, hi, wup, wdn, o.cnt, o.wsum,
                                   o.fsum, o.wfsum, first, count, p->stream));
  }
  return 0;
}
// the condition, the bounds, the thresholds, the outputs and the value tracers of a call, for the plan forms (ntracers of
// the plan) and the array forms alike; the thresholds are checked as given (rounding to fp32 is monotone); without fsum and
// wfsum the range is not looked at
static int level_draft_args(const char* what, int ntracers, int tc, const void* lo, const void* hi, double wup, double wdn,
                            const LevelDraftOut& o, int first, int count) {
  if (tc < -1 || tc >= ntracers) return set_err(MPDATA_EINVAL, "%s: condition tracer tc %d outside [-1, %d)", what, tc, ntracers);
  if (tc < 0 && (lo || hi)) return set_err(MPDATA_EINVAL, "%s: lo or hi given without a condition tracer (tc = -1)", what);
  if (wup != wup || wdn != wdn) return set_err(MPDATA_EINVAL, "%s: a threshold is a NaN", what);
  if (wdn > wup) return set_err(MPDATA_EINVAL, "%s: wdn %g > wup %g", what, wdn, wup);
  if (!o.cnt && !o.wsum && !o.fsum && !o.wfsum) return set_err(MPDATA_EINVAL, "%s: cnt, wsum, fsum and wfsum are all NULL", what);
  if ((o.fsum || o.wfsum) && (first < 0 || count < 1 || first > ntracers - count))
    return set_err(MPDATA_EINVAL, "%s: tracer range [%d, %lld) outside the %d tracers", what, first, (long long)first + count, ntracers);
  return 0;
}
static int plan_level_draft_check(const char* what, const mpdata_plan* p, int64_t sl0, int64_t n, int tc, const void* lo, const void* hi,
                                  double wup, double wdn, const LevelDraftOut& o, int first, int count, int eb) {
  int rc = block_range(what, p, sl0, n);
  if (rc) return rc;
  rc = level_draft_args(what, p->ntracers, tc, lo, hi, wup, wdn, o, first, count);
  return rc ? rc : plan_state(what, p, eb, false, true);
}
int mpdata_plan_level_draft_device(mpdata_plan* p, int64_t sl0, int64_t n, int tc, const void* lo, const void* hi, double wup, double wdn,
                                   void* cnt, void* wsum, void* fsum, void* wfsum, int first_tracer, int ntracers) {
  const LevelDraftOut o = {cnt, wsum, fsum, wfsum};
  const int rc = plan_level_draft_check("mpdata_plan_level_draft_device", p, sl0, n, tc, lo, hi, wup, wdn, o, first_tracer, ntracers, 0);
  if (rc) return rc;
  DevGuard g(p->device);
  return plan_level_draft(p, sl0, n, tc, lo, hi, wup, wdn, o, first_tracer, ntracers);
}
static int plan_level_draft_host(mpdata_plan* p, int64_t sl0, int64_t n, int tc, const void* lo, const void* hi, double wup, double wdn,
                                 const LevelDraftOut& o, int eb) {
  int rc = plan_level_draft_check("mpdata_plan_level_draft", p, sl0, n, tc, lo, hi, wup, wdn, o, 0, p ? p->ntracers : 0, eb);
  if (rc) return rc;
  DevGuard g(p->device);
  const size_t kb = (size_t)n * (p->nz - 1) * eb, cb = kb * MPDATA_LEVEL_DRAFT_CLASSES;
  HostArr a[6] = {{lo, kb, false}, {hi, kb, false}, {o.cnt, cb, true}, {o.wsum, cb, true}, {o.fsum, cb * p->ntracers, true},
                  {o.wfsum, cb * p->ntracers, true}};
  rc = stage_in(p, a);
  const LevelDraftOut d = {a[2].dev, a[3].dev, a[4].dev, a[5].dev};
  if (!rc) rc = plan_level_draft(p, sl0, n, tc, a[0].dev, a[1].dev, wup, wdn, d, 0, p->ntracers);
  return rc ? rc : stage_out(p, a);
}
int mpdata_plan_level_draft(mpdata_plan* p, int64_t sl0, int64_t n, int tc, const double* lo, const double* hi, double wup, double wdn,
                            double* cnt, double* wsum, double* fsum, double* wfsum) {
  return plan_level_draft_host(p, sl0, n, tc, lo, hi, wup, wdn, {cnt, wsum, fsum, wfsum}, 8);
}
int mpdata_plan_level_draft_f32(mpdata_plan* p, int64_t sl0, int64_t n, int tc, const float* lo, const float* hi, double wup, double wdn,
                                float* cnt, float* wsum, float* fsum, float* wfsum) {
  return plan_level_draft_host(p, sl0, n, tc, lo, hi, wup, wdn, {cnt, wsum, fsum, wfsum}, 4);
}
// the same on reference-layout device arrays (arguments checked before any device call): asynchronous.  w is required; f
// only where the condition or a sum reads it
static int level_draft_array(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, const void* f, const void* w, int tc,
                             const void* lo, const void* hi, double wup, double wdn, const LevelDraftOut& o, int first, int count,
                             void* stream, int eb) {
  const char* const what = "mpdata_level_draft_device";
  int rc = array_sizes(what, ncrms, nx, nz, &ntracers);
  if (rc) return rc;
  rc = array_block(what, ncrms, sl0, n);
  if (rc) return rc;
  if (!w) return set_err(MPDATA_EINVAL, "%s: null w", what);
  if (!f && (tc >= 0 || o.fsum || o.wfsum)) return set_err(MPDATA_EINVAL, "%s: null f", what);
  rc = level_draft_args(what, ntracers, tc, lo, hi, wup, wdn, o, first, count);
  if (rc) return rc;
  HIP_TRY(mpdata_level_draft_ref(f, w, eb, ncrms, sl0, n, nx, nz - 1, ntracers, tc, lo, hi, wup, wdn, o.cnt, o.wsum, o.fsum, o.wfsum, first,
                                 count, (hipStream_t)stream));
  return 0;
}
int mpdata_level_draft_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, const double* f, const double* w, int tc,
                              const double* lo, const double* hi, double wup, double wdn, double* cnt, double* wsum, double* fsum,
                              double* wfsum, int first_tracer, int ntr, void* stream) {
  return level_draft_array(ncrms, nx, nz, ntracers, sl0, n, f, w, tc, lo, hi, wup, wdn, {cnt, wsum, fsum, wfsum}, first_tracer, ntr, stream, 8);
}
int mpdata_level_draft_f32_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, const float* f, const float* w, int tc,
                                  const float* lo, const float* hi, double wup, double wdn, float* cnt, float* wsum, float* fsum,
                                  float* wfsum, int first_tracer, int ntr, void* stream) {
  return level_draft_array(ncrms, nx, nz, ntracers, sl0, n, f, w, tc, lo, hi, wup, wdn, {cnt, wsum, fsum, wfsum}, first_tracer, ntr, stream, 4);
}

}  // extern "C"
