// mpdata_plan.hip -- plans: the device-resident state of one problem behind the C-ABI (include/mpdata_hip.h 3; the calls on
// a block of instances, 3g .. 3m, are in mpdata_plan_blocks.hip).
// A plan owns the device state of one problem (what the OpenACC `enter data pcreate` of the
// reference does, :105, :280, :662) on the device that was current when it was created; every
// plan call switches to that device and back.  Variant and layout are fixed at creation.
// fp64 plans with nz <= 64 keep the arrays in the wave-major layout of
// mpdata_kernel_wm_body.h and convert in upload / download / import / export; other plans
// (fp32; nz > 64) keep the reference layout and run the x-/k-marching kernels.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "mpdata_plan_priv.h"
#include "mpdata_windows.h"

using namespace mpd;

namespace {
// EXACT, bit-identical flux: the plan kernels store the upwind sum as flux and PARK the nx limited vertical fluxes of
// every lane ([tracer][tile][column][lane], mpdata_kernel_wm_body.h); this adds them, one by one in the reference's
// order i = 1 .. nx (:624), onto that sum.  A wave per (tracer, tile), lane -> (instance, level) as in the kernels.
// R2 = double, or float2 for fp32 plans (two adjacent instances per lane; no contraction: this file is built with
// -ffp-contract=off).
template <typename R2>
__global__ void __launch_bounds__(256) flux_finish_kernel(R2* flux, const R2* park, int ntiles, int nx, int nzm, int lps,
                                                          long long flux_tstride, int ntr, int nkw) {
  const int lane = threadIdx.x & 63;
  const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);   // wave = (tracer * ntiles + tile) * nkw + wave of the instance
  if (w >= (long long)ntr * ntiles * nkw) return;
  const int h = (int)(w % nkw);
  const long long tt = w / nkw;
  const int tr = (int)(tt / ntiles), tile = (int)(tt % ntiles);
  int s_l = lane / lps, kk = lane % lps, chunk = (64 / lps) * nzm;
  if (lps > 64) {   // nz > 64: the wave's 64-level window and the part of it the plan kernel stores (mpdata_kernel_wm_body.h: koff, out_ok)
    const int nz = nzm + 1;
    const int koff = min(58 * h, max(0, (nz - 64 + 1) & ~1));
    s_l = 0; kk = lane + koff; chunk = nzm;
    const int k = kk + 1;
    if (!((h == 0 || k >= 58 * h + 4) && (h + 1 == nkw || k <= 58 * h + 61))) return;
  }
  if (kk >= nzm) return;
  R2* fp = flux + (long long)tr * flux_tstride + (long long)tile * chunk + s_l * nzm + kk;
  const R2* pp = park + w * ((long long)nx * 64) + lane;
  R2 acc = *fp;
  for (int i = 0; i < nx; ++i) {
    const R2 t = pp[(long long)i * 64];
    if constexpr (sizeof(R2) == 8 && alignof(R2) == 8 && !std::is_same<R2, double>::value) { acc.x = acc.x + t.x; acc.y = acc.y + t.y; }
    else acc = acc + t;
  }
  *fp = acc;
}

}  // namespace

// (the helpers mpdata_plan_blocks.hip shares are declared in mpdata_plan_priv.h; the others are static)
namespace mpd {

// conversion jobs of a wave-major plan: which = 0 f, 1 u, 2 w, 3 rho, 4 rhow, 5 adz, 6 flux
MpdataLayoutJob wm_job(const mpdata_plan* p, int which, void* ref, int first_tracer, int ntr) {
  MpdataLayoutJob j;
  const int nzm = p->nz - 1, nx = p->nx;
  // (fp32 plans: every array seen as wm_ncrms = ncrms / 2 pairs of adjacent instances, 8 bytes each; with an odd ncrms
  //  the reference side is counted in reals instead -- lref -- and only mpdata_layout_convert_odd takes the job whole)
  const long long lref = p->odd ? p->ncrms : p->wm_ncrms;
  j.ref = ref; j.ncrms = lref; j.nlev = nzm; j.ntr = 1; j.slp = p->slp; j.ntiles = p->ntiles;
  j.chunk = p->chunk; j.ref_tstride = 0; j.prv_tstride = 0; j.prv_col0 = 0;
  j.main_e = which <= 2 ? p->main_e : 0;   // f, u, w are split into line-aligned part + rest
  j.ncol_p = nx + 6;
  j.ref_colmul = 1;
  switch (which) {
    case 0:
      j.prv = (double*)p->pf + (long long)first_tracer * p->ntiles * p->tile_elems;
      j.ncols = nx + 6; j.ref_levmul = nx + 6; j.prv_tile_stride = p->tile_elems;
      j.ntr = ntr; j.ref_tstride = lref * (nx + 6) * nzm; j.prv_tstride = (long long)p->ntiles * p->tile_elems;
      break;
    case 1: j.prv = p->pu; j.ncols = nx + 5; j.ref_levmul = nx + 5; j.prv_col0 = 1; j.prv_tile_stride = p->tile_elems; break;
    case 2: j.prv = p->pw; j.ncols = nx + 4; j.ref_levmul = nx + 4; j.prv_col0 = 1; j.prv_tile_stride = p->tile_elems; break;
    case 3: case 4: case 5:   // kc = [tile][rho, adz, rhow][chunk]
      j.prv = p->pkc; j.ncols = 1; j.ref_colmul = 0; j.ref_levmul = 1; j.prv_tile_stride = 3 * p->chunk;
      j.prv_col0 = which == 3 ? 0 : (which == 5 ? 1 : 2);
      break;
    default:
      j.prv = (double*)p->pflux + (long long)first_tracer * p->ntiles * p->chunk;
      j.ncols = 1; j.ref_colmul = 0; j.ref_levmul = 1; j.prv_tile_stride = p->chunk;
      j.ntr = ntr; j.ref_tstride = lref * p->nz; j.prv_tstride = (long long)p->ntiles * p->chunk;
      break;
  }
  return j;
}

// lanes per instance of the wave-major kernels; 128 = an instance wider than a wave (65 <= nz <= 238: several waves
// per instance, mpdata_kernel_wm_body.h "KS"; the layout kernels hold a column of one instance group in LDS: nzm <= 126)
#define MPDATA_WM_NZ_MAX 238   // 64 + 3 * 58: four windows = the four waves of a workgroup
static int wm_lps_for(int nz) { return nz <= 8 ? 8 : nz <= 16 ? 16 : nz <= 32 ? 32 : nz <= 64 ? 64 : nz <= MPDATA_WM_NZ_MAX ? 128 : 0; }
static int wm_nkw_for(int nz) { return nz <= 64 ? 1 : 1 + (nz - 64 + 57) / 58; }
// nz > 64: lanes of the last window where it is a share of a wave (16: the window needs <= 16 levels, 32: <= 32; else 0 = a
// wave of its own); MPDATA_KS_TAIL=0: never (A/B)
static int wm_lwt_for(int nz) {
  static const bool off = getenv("MPDATA_KS_TAIL") && !strcmp(getenv("MPDATA_KS_TAIL"), "0");
  if (nz <= 64 || off || wm_nkw_for(nz) != 2) return 0;   // (three windows: a 9-wave workgroup would cap the two-waves-per-SIMD forms' registers)
  const int need = nz - 58 * (wm_nkw_for(nz) - 1);
  return need <= 16 ? 16 : need <= 32 ? 32 : 0;
}

// ---- windowed plans: the inner plan follows the outer one's stream and boundary mode
static mpdata_plan* win_inner(mpdata_plan* p) {
  p->inner->stream = p->stream;
  p->inner->boundary = p->boundary;
  return p->inner;
}
// one array of instances [sl0, sl0 + n) between a tall reference-layout array of leading dimension n and the windows
static MpdataWindowJob win_job(const mpdata_plan* p, int which, void* ref, int64_t sl0, int64_t n, int first_tracer, int ntr) {
  MpdataWindowJob b;
  b.j = wm_job(p->inner, which, ref, first_tracer, ntr);
  b.j.ref_tstride = which == 0 ? (long long)n * (p->nx + 6) * (p->nz - 1) : which == 6 ? (long long)n * p->nz : 0;
  b.sl0 = sl0; b.n = n; b.ncrms = p->ncrms; b.ipe = 8 / p->eb; b.nz = p->nz;
  return b;
}

int plan_check(const mpdata_plan* p, int eb) {
  if (!p) return set_err(MPDATA_EINVAL, "null plan");
  if (p->eb != eb) return set_err(MPDATA_ESTATE, "plan precision (%d-byte reals) does not match the call", p->eb);
  return 0;
}
int tracer_range(const mpdata_plan* p, int first, int count) {
  if (first < 0 || count < 1 || first + count > p->ntracers)
    return set_err(MPDATA_EINVAL, "tracer range [%d, %d) outside the plan's %d tracers", first, first + count, p->ntracers);
  return 0;
}

// The reference-layout staging buffer of a wave-major plan (one tracer of f, or u / w): only host
// transfers need it, so it is allocated by the first of them (a plan that is only ever fed from
// device arrays -- bench.py keeps one per field set -- never pays its 538 MB).
static int plan_stage(mpdata_plan* p) {
  if (p->stage) return 0;
  HIP_TRY(hipMalloc(&p->stage, p->stage_elems * p->eb));
  return 0;
}

// MPDATA_LAYOUT_LEGACY=1: the round-2 conversion kernel (one workgroup per column) for f, u, w as well (A/B)
bool legacy_convert() {
  static const bool v = getenv("MPDATA_LAYOUT_LEGACY") != nullptr;
  return v;
}

// fp32 plans with an odd ncrms: the phantom half and the padding pairs of array `which` := the plan's last instance
// (tracers [first, first + ntr) of f / flux).  Behind every import that replaced that instance in single reals.
int plan_phantom(mpdata_plan* p, int which, int first, int ntr) {
  if (!p->odd) return 0;
  HIP_TRY(mpdata_layout_refresh_phantom(wm_job(p, which, nullptr, first, ntr), p->ncrms - 1, p->stream));
  return 0;
}

// Windowed plans: tall reference-layout arrays of instances [sl0, sl0 + n) (leading dimension n; host arrays: the whole
// plan only) -> the windows (split: every level every window holds, so a whole import of f leaves fresh seams; after a
// block import the seams of the plan are as fresh as they were).  flux is also kept tall (level nz).
static int win_import(mpdata_plan* p, int64_t sl0, int64_t n, const void* f, const void* u, const void* w, const void* rho,
                      const void* rhow, const void* adz, const void* flux, int first, int count, bool dev) {
  const int eb = p->eb;
  const bool whole = n == p->ncrms, last = sl0 + n == p->ncrms;
  const size_t f1 = (size_t)n * (p->nx + 6) * (p->nz - 1);   // elements of one tracer of f
  win_inner(p);
  if (!dev) {
    const int rs = plan_stage(p);
    if (rs) return rs;
  }
  auto one = [&](int which, const void* src, size_t elems, int tr, int ntr) -> int {
    void* ref = const_cast<void*>(src);
    if (!dev) {
      HIP_TRY(hipMemcpyAsync(p->stage, src, elems * eb, hipMemcpyHostToDevice, p->stream));
      ref = p->stage;
    }
    HIP_TRY(mpdata_window_convert(win_job(p, which, ref, sl0, n, tr, ntr), true, p->stream));
    return last ? plan_phantom(p->inner, which, tr, ntr) : 0;   // (an odd number of windows: the split moves real ones only)
  };
  int rc = 0;
  if (f) {
    memset(p->halo_ok + first, 0, (size_t)count);   // (imported halos are not trusted: a periodic plan wraps again)
    if (dev) rc = one(0, f, 0, first, count);
    else for (int t = 0; t < count && !rc; ++t) rc = one(0, (const char*)f + (size_t)t * f1 * eb, f1, first + t, 1);
    if (!rc && whole) memset(p->seam_ok + first, 1, (size_t)count);
  }
  if (!rc && u) { rc = one(1, u, p->sz.u, 0, 1); if (!rc && whole) p->have_u = true; }
  if (!rc && w) { rc = one(2, w, p->sz.w, 0, 1); if (!rc && whole) p->have_w = true; }
  if (!rc && rho) rc = one(3, rho, p->sz.k, 0, 1);
  if (!rc && rhow) rc = one(4, rhow, p->sz.kz, 0, 1);
  if (!rc && adz) rc = one(5, adz, p->sz.k, 0, 1);
  if (!rc && flux) {
    char* fr = (char*)p->flux_ref + (size_t)first * p->sz.kz * eb;
    if (whole) {
      HIP_TRY(hipMemcpyAsync(fr, flux, p->sz.kz * count * eb, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, p->stream));
      HIP_TRY(mpdata_window_convert(win_job(p, 6, fr, 0, n, first, count), true, p->stream));
      rc = plan_phantom(p->inner, 6, first, count);
    } else {
      HIP_TRY(mpdata_layout_copy_rows(fr + (size_t)sl0 * eb, flux, eb, n, (long long)p->nz * count, p->ncrms, n, p->stream));
      HIP_TRY(mpdata_window_convert(win_job(p, 6, const_cast<void*>(flux), sl0, n, first, count), true, p->stream));
      if (last) rc = plan_phantom(p->inner, 6, first, count);
    }
  }
  return rc;
}

// ... and back (merge: the owned levels of every window; flux level nz from the tall copy).  The caller has wrapped
// the halos of a periodic plan.
static int win_export(mpdata_plan* p, int64_t sl0, int64_t n, void* f, void* flux, int first, int count, bool dev) {
  const int eb = p->eb, nz = p->nz, nzm = nz - 1;
  const bool whole = n == p->ncrms;
  const size_t f1 = (size_t)n * (p->nx + 6) * nzm;
  win_inner(p);
  if (f) {
    if (dev) {
      HIP_TRY(mpdata_window_convert(win_job(p, 0, f, sl0, n, first, count), false, p->stream));
    } else {
      const int rs = plan_stage(p);
      if (rs) return rs;
      for (int t = 0; t < count; ++t) {
        HIP_TRY(mpdata_window_convert(win_job(p, 0, p->stage, sl0, n, first + t, 1), false, p->stream));
        HIP_TRY(hipMemcpyAsync((char*)f + (size_t)t * f1 * eb, p->stage, f1 * eb, hipMemcpyDeviceToHost, p->stream));
      }
    }
  }
  if (flux) {
    char* fr = (char*)p->flux_ref + (size_t)first * p->sz.kz * eb;
    if (whole) {
      HIP_TRY(mpdata_window_convert(win_job(p, 6, fr, 0, n, first, count), false, p->stream));
      HIP_TRY(hipMemcpyAsync(flux, fr, p->sz.kz * count * eb, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, p->stream));
    } else {
      HIP_TRY(mpdata_window_convert(win_job(p, 6, flux, sl0, n, first, count), false, p->stream));
      HIP_TRY(mpdata_layout_copy_rows((char*)flux + (size_t)nzm * n * eb, fr + ((size_t)nzm * p->ncrms + (size_t)sl0) * eb, eb, n, count,
                                      (long long)n * nz, (long long)p->ncrms * nz, p->stream));
    }
  }
  return 0;
}

// Windowed plans: the seam refresh in front of a run -- one launch over the span of tracers [first, first + count)
// whose seams a run has left stale; nothing right after an import.
int plan_seams(mpdata_plan* p, int first, int count) {
  if (!p->inner) return 0;
#ifdef MPDATA_TALL_NOSEAMS   // diagnostic builds only: no refresh, WRONG results from the second run on (docs/EXPERIMENTS.md)
  return 0;
#endif
  int lo = first, hi = first + count;
  while (lo < hi && p->seam_ok[lo]) ++lo;
  while (hi > lo && p->seam_ok[hi - 1]) --hi;
  if (lo == hi) return 0;
  win_inner(p);
  HIP_TRY(mpdata_window_seams(win_job(p, 0, nullptr, 0, p->ncrms, lo, hi - lo), p->stream));
  const int rc = plan_phantom(p->inner, 0, lo, hi - lo);   // (the refresh acts on real windows: the phantom follows the last one)
  if (rc) return rc;
  memset(p->seam_ok + lo, 1, (size_t)(hi - lo));
  return 0;
}

// Arrays in the reference layout -> the plan.  `dev` says where the pointers live.  Null
// pointers are skipped (the plan keeps what it has).  f / flux cover `count` tracers.
static int plan_import(mpdata_plan* p, const void* f, const void* u, const void* w, const void* rho,
                       const void* rhow, const void* adz, const void* flux, int first, int count, bool dev) {
  const int eb = p->eb;
  const size_t f1 = p->sz.f / p->ntracers;  // elements of one tracer of f
  const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  if (p->inner) return win_import(p, 0, p->ncrms, f, u, w, rho, rhow, adz, flux, first, count, dev);
  if (f) memset(p->halo_ok + first, 0, (size_t)count);   // (imported halos are not trusted: a periodic plan wraps again)
  if (p->layout == MPDATA_LAYOUT_REFERENCE) {
    if (f) HIP_TRY(hipMemcpyAsync((char*)p->f + first * f1 * eb, f, f1 * count * eb, kind, p->stream));
    if (u) { HIP_TRY(hipMemcpyAsync(p->u, u, p->sz.u * eb, kind, p->stream)); p->have_u = true; }
    if (w) { HIP_TRY(hipMemcpyAsync(p->w, w, p->sz.w * eb, kind, p->stream)); p->have_w = true; }
    if (rho) HIP_TRY(hipMemcpyAsync(p->rho, rho, p->sz.k * eb, kind, p->stream));
    if (rhow) HIP_TRY(hipMemcpyAsync(p->rhow, rhow, p->sz.kz * eb, kind, p->stream));
    if (adz) HIP_TRY(hipMemcpyAsync(p->adz, adz, p->sz.k * eb, kind, p->stream));
    if (flux) HIP_TRY(hipMemcpyAsync((char*)p->flux + first * p->sz.kz * eb, flux, p->sz.kz * count * eb, kind, p->stream));
    return 0;
  }
  // wave-major: device sources are converted in place, host sources go through the staging
  // buffer one array (one tracer of f) at a time
  if (!dev) {
    const int rs = plan_stage(p);
    if (rs) return rs;
  }
  // f, u, w (many columns, split chunks): the column-walking kernel; the small arrays: the per-column one
  auto conv = [&](int which, void* ref, int tr, int ntr) -> int {
    const MpdataLayoutJob j = wm_job(p, which, ref, tr, ntr);
    if (p->odd) {
      HIP_TRY(mpdata_layout_convert_odd(&j, 1, true, p->stream));
    } else if (which <= 2 && !legacy_convert()) {
      const hipError_t e = mpdata_layout_import_rows(&j, 1, p->stream);   // (row segments through LDS-DMA where possible)
      if (e == hipErrorNotSupported) HIP_TRY(mpdata_layout_convert_cols(&j, 1, true, p->stream));
      else HIP_TRY(e);
    } else {
      HIP_TRY(mpdata_layout_convert(j, 8, true, p->stream));
    }
    return 0;
  };
  auto one = [&](int which, const void* src, size_t elems, int tr) -> int {
    void* ref = const_cast<void*>(src);
    if (!dev) {
      HIP_TRY(hipMemcpyAsync(p->stage, src, elems * eb, hipMemcpyHostToDevice, p->stream));
      ref = p->stage;
    }
    return conv(which, ref, tr, 1);
  };
  int rc = 0;
  if (f) {
    if (dev) {
      rc = conv(0, const_cast<void*>(f), first, count);
    } else {
      for (int t = 0; t < count && !rc; ++t) rc = one(0, (const char*)f + (size_t)t * f1 * eb, f1, first + t);
    }
  }
  if (!rc && u && w && dev && !legacy_convert()) {   // u and w of a device import: ONE launch
    const MpdataLayoutJob j2[2] = {wm_job(p, 1, const_cast<void*>(u), 0, 1), wm_job(p, 2, const_cast<void*>(w), 0, 1)};
    const hipError_t e = p->odd ? mpdata_layout_convert_odd(j2, 2, true, p->stream) : mpdata_layout_import_rows(j2, 2, p->stream);
    if (e == hipErrorNotSupported) HIP_TRY(mpdata_layout_convert_cols(j2, 2, true, p->stream));
    else HIP_TRY(e);
    p->have_u = p->have_w = true;
  } else {
    if (!rc && u) { rc = one(1, u, p->sz.u, 0); if (!rc) p->have_u = true; }
    if (!rc && w) { rc = one(2, w, p->sz.w, 0); if (!rc) p->have_w = true; }
  }
  if (!rc && rho) rc = one(3, rho, p->sz.k, 0);
  if (!rc && rhow) rc = one(4, rhow, p->sz.kz, 0);
  if (!rc && adz) rc = one(5, adz, p->sz.k, 0);
  if (!rc && flux) {
    // kept twice: in the reference layout (level nz is carried through to the export) and in the
    // private array (a tracer that is never run exports what was imported)
    void* fr = (char*)p->flux_ref + (size_t)first * p->sz.kz * eb;
    HIP_TRY(hipMemcpyAsync(fr, flux, p->sz.kz * count * eb, kind, p->stream));
    const MpdataLayoutJob j = wm_job(p, 6, fr, first, count);
    if (p->odd) HIP_TRY(mpdata_layout_convert_odd(&j, 1, true, p->stream));
    else HIP_TRY(mpdata_layout_convert(j, 8, true, p->stream));
  }
  return rc;
}

// Periodic plans: f's halo columns of tracers [first, first + count) := copies of the interior, where they are not
// already (mpdata_layout_periodic_halo_*: one launch over the unmarked span of the range); a no-op in GIVEN mode.
int plan_wrap_f(mpdata_plan* p, int first, int count) {
  if (p->boundary != MPDATA_BOUNDARY_PERIODIC) return 0;
  if (p->inner) return plan_wrap_f(win_inner(p), first, count);   // (every window, every level it holds: halo_ok is shared)
  int lo = first, hi = first + count;
  while (lo < hi && p->halo_ok[lo]) ++lo;
  while (hi > lo && p->halo_ok[hi - 1]) --hi;
  if (lo == hi) return 0;
  if (p->layout == MPDATA_LAYOUT_WAVEMAJOR) {
    HIP_TRY(mpdata_layout_periodic_halo_wm(wm_job(p, 0, nullptr, lo, hi - lo), p->stream));
  } else {
    const size_t f1 = p->sz.f / p->ntracers;
    HIP_TRY(mpdata_layout_periodic_halo_ref((char*)p->f + (size_t)lo * f1 * p->eb, p->eb, p->ncrms, p->nx, p->nx + 6, 2, p->nz - 1,
                                            hi - lo, -2, p->nx + 3, p->stream));
  }
  memset(p->halo_ok + lo, 1, (size_t)(hi - lo));
  return 0;
}

static int plan_export(mpdata_plan* p, void* f, void* flux, int first, int count, bool dev) {
  const int eb = p->eb;
  if (f) {   // (periodic plans hand out wrapped halos)
    const int rc = plan_wrap_f(p, first, count);
    if (rc) return rc;
  }
  const size_t f1 = p->sz.f / p->ntracers;
  const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (p->inner) return win_export(p, 0, p->ncrms, f, flux, first, count, dev);
  if (p->layout == MPDATA_LAYOUT_REFERENCE) {
    if (f) HIP_TRY(hipMemcpyAsync(f, (char*)p->f + first * f1 * eb, f1 * count * eb, kind, p->stream));
    if (flux) HIP_TRY(hipMemcpyAsync(flux, (char*)p->flux + first * p->sz.kz * eb, p->sz.kz * count * eb, kind, p->stream));
    return 0;
  }
  auto conv_out = [&](void* ref, int tr, int ntr) -> int {
    const MpdataLayoutJob j = wm_job(p, 0, ref, tr, ntr);
    if (p->odd) HIP_TRY(mpdata_layout_convert_odd(&j, 1, false, p->stream));
    else if (!legacy_convert()) HIP_TRY(mpdata_layout_convert_cols(&j, 1, false, p->stream));
    else HIP_TRY(mpdata_layout_convert(j, 8, false, p->stream));
    return 0;
  };
  if (f) {
    if (dev) {
      const int rc = conv_out(f, first, count);
      if (rc) return rc;
    } else {
      const int rs = plan_stage(p);
      if (rs) return rs;
      for (int t = 0; t < count; ++t) {
        const int rc = conv_out(p->stage, first + t, 1);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync((char*)f + (size_t)t * f1 * eb, p->stage, f1 * eb, hipMemcpyDeviceToHost, p->stream));
      }
    }
  }
  if (flux) {
    // levels 1..nzm from the kernel's result; level nz is whatever was uploaded (the reference
    // never writes it, :541, :624)
    void* fr = (char*)p->flux_ref + (size_t)first * p->sz.kz * eb;
    const MpdataLayoutJob j = wm_job(p, 6, fr, first, count);
    if (p->odd) HIP_TRY(mpdata_layout_convert_odd(&j, 1, false, p->stream));
    else HIP_TRY(mpdata_layout_convert(j, 8, false, p->stream));
    HIP_TRY(hipMemcpyAsync(flux, fr, p->sz.kz * count * eb, kind, p->stream));
  }
  return 0;
}

// ---- Blocks of instances (include/mpdata_hip.h 3d): instances [sl0, sl0 + n) of the plan <-> reference-layout DEVICE
// arrays of leading dimension n.  Wave-major plans: the block kernel of mpdata_layout.hip, one launch per array over
// the tiles the block touches; reference-layout plans: the block is a strided slab of every array.
MpdataBlockJob wm_block_job(const mpdata_plan* p, int which, void* ref, int64_t sl0, int64_t n, int first_tracer, int ntr) {
  MpdataBlockJob b;
  b.j = wm_job(p, which, ref, first_tracer, ntr);
  b.j.ref_tstride = which == 0 ? (long long)n * (p->nx + 6) * (p->nz - 1) : which == 6 ? (long long)n * p->nz : 0;
  // (an odd fp32 plan: the phantom counts as an instance no block contains -- the kernel then neither fills nor exports
  //  it, and its padding rule never writes a wrong half; plan_phantom restores the invariant behind the import)
  b.sl0 = sl0; b.n = n; b.ncrms = p->ncrms + (p->odd ? 1 : 0); b.ipe = 8 / p->eb;
  return b;
}

static int plan_import_block(mpdata_plan* p, int64_t sl0, int64_t n, const void* f, const void* u, const void* w, const void* rho,
                             const void* rhow, const void* adz, const void* flux, int first, int count) {
  const int eb = p->eb, nx = p->nx, nz = p->nz, nzm = nz - 1;
  if (p->inner) return win_import(p, sl0, n, f, u, w, rho, rhow, adz, flux, first, count, true);
  if (f) memset(p->halo_ok + first, 0, (size_t)count);   // (as a whole import: a periodic plan wraps these tracers again)
  // the slab of rows x n reals at instance sl0 of a reference-layout array of the plan
  auto slab = [&](void* dst, const void* src, long long rows) -> int {
    HIP_TRY(mpdata_layout_copy_rows((char*)dst + (size_t)sl0 * eb, src, eb, n, rows, p->ncrms, n, p->stream));
    return 0;
  };
  int rc = 0;
  if (p->layout == MPDATA_LAYOUT_REFERENCE) {
    const size_t f1 = p->sz.f / p->ntracers;
    if (f) rc = slab((char*)p->f + first * f1 * eb, f, (long long)(nx + 6) * nzm * count);
    if (!rc && u) rc = slab(p->u, u, (long long)(nx + 5) * nzm);
    if (!rc && w) rc = slab(p->w, w, (long long)(nx + 4) * nz);
    if (!rc && rho) rc = slab(p->rho, rho, nzm);
    if (!rc && rhow) rc = slab(p->rhow, rhow, nz);
    if (!rc && adz) rc = slab(p->adz, adz, nzm);
    if (!rc && flux) rc = slab((char*)p->flux + first * p->sz.kz * eb, flux, (long long)nz * count);
    return rc;
  }
  auto conv = [&](int which, const void* ref, int tr, int ntr) -> int {
    HIP_TRY(mpdata_layout_convert_block(wm_block_job(p, which, const_cast<void*>(ref), sl0, n, tr, ntr), true, p->stream));
    return sl0 + n == p->ncrms ? plan_phantom(p, which, tr, ntr) : 0;
  };
  if (f) rc = conv(0, f, first, count);
  if (!rc && u) rc = conv(1, u, 0, 1);
  if (!rc && w) rc = conv(2, w, 0, 1);
  if (!rc && rho) rc = conv(3, rho, 0, 1);
  if (!rc && rhow) rc = conv(4, rhow, 0, 1);
  if (!rc && adz) rc = conv(5, adz, 0, 1);
  if (!rc && flux) {   // kept twice (plan_import): the reference-layout copy carries level nz
    rc = slab((char*)p->flux_ref + (size_t)first * p->sz.kz * eb, flux, (long long)nz * count);
    if (!rc) rc = conv(6, flux, first, count);
  }
  return rc;
}

// f, flux: device arrays of the block
static int plan_export_block(mpdata_plan* p, int64_t sl0, int64_t n, void* f, void* flux, int first, int count) {
  const int eb = p->eb, nx = p->nx, nz = p->nz, nzm = nz - 1;
  auto slab = [&](void* dst, const void* src, long long rows) -> int {
    HIP_TRY(mpdata_layout_copy_rows(dst, (const char*)src + (size_t)sl0 * eb, eb, n, rows, n, p->ncrms, p->stream));
    return 0;
  };
  int rc = 0;
  if (p->inner) {
    rc = win_export(p, sl0, n, f, flux, first, count, true);
  } else if (p->layout == MPDATA_LAYOUT_REFERENCE) {
    const size_t f1 = p->sz.f / p->ntracers;
    if (f) rc = slab(f, (char*)p->f + first * f1 * eb, (long long)(nx + 6) * nzm * count);
    if (!rc && flux) rc = slab(flux, (char*)p->flux + first * p->sz.kz * eb, (long long)nz * count);
  } else {
    if (f) HIP_TRY(mpdata_layout_convert_block(wm_block_job(p, 0, f, sl0, n, first, count), false, p->stream));
    if (flux) {
      // levels 1..nzm from the private array, level nz from the reference-layout copy (plan_export)
      HIP_TRY(mpdata_layout_convert_block(wm_block_job(p, 6, flux, sl0, n, first, count), false, p->stream));
      const char* fr = (const char*)p->flux_ref + ((size_t)first * p->sz.kz + (size_t)nzm * p->ncrms + (size_t)sl0) * eb;
      HIP_TRY(mpdata_layout_copy_rows((char*)flux + (size_t)nzm * n * eb, fr, eb, n, count, (long long)n * nz,
                                      (long long)p->ncrms * nz, p->stream));
    }
  }
  if (rc) return rc;
  // periodic plans hand out wrapped halos: where the plan's own are stale, the BLOCK's copy is wrapped (the same bits
  // as a refresh of the plan followed by the read-back, at the cost of the block; the plan's state is not touched)
  if (f && p->boundary == MPDATA_BOUNDARY_PERIODIC) {
    bool stale = false;
    for (int t = first; t < first + count; ++t) stale = stale || !p->halo_ok[t];
    if (stale) HIP_TRY(mpdata_layout_periodic_halo_ref(f, eb, n, nx, nx + 6, 2, nzm, count, -2, nx + 3, p->stream));
  }
  return 0;
}

// argument checks of the block entry points that need nothing of the plan but its sizes
int block_range(const char* what, const mpdata_plan* p, int64_t sl0, int64_t n) {
  if (!p) return set_err(MPDATA_EINVAL, "%s: null plan", what);
  if (n < 1) return set_err(MPDATA_EINVAL, "%s: a block of n = %lld instances", what, (long long)n);
  if (sl0 < 0) return set_err(MPDATA_EINVAL, "%s: first instance sl0 = %lld", what, (long long)sl0);
  if (p->multi)
    return set_err(MPDATA_EUNSUPPORTED, "%s on a multi-GPU handle: a block is taken by the single-device plan of a shard "
                                        "(mpdata_plan_shard_plan) with a shard-local sl0", what);
  if (sl0 > p->ncrms - n)
    return set_err(MPDATA_EINVAL, "%s: instances [%lld, %lld) outside the plan's %lld", what, (long long)sl0, (long long)(sl0 + n),
                   (long long)p->ncrms);
  return 0;
}
// the plan's block staging buffer (device memory the host forms of the block calls go through): at least `need` bytes
int plan_bstage(mpdata_plan* p, size_t need) {
  if (p->bstage_bytes >= need) return 0;
  HIP_TRY(hipStreamSynchronize(p->stream));
  if (p->bstage) (void)hipFree(p->bstage);
  p->bstage = nullptr; p->bstage_bytes = 0;
  HIP_TRY(hipMalloc(&p->bstage, need));
  p->bstage_bytes = need;
  return 0;
}

}  // namespace mpd

extern "C" {

static int plan_create(int64_t ncrms, int nx, int nz, int ntracers, mpdata_plan** plan, int eb, int var_in = -1) {
  if (!plan) return set_err(MPDATA_EINVAL, "null plan pointer");
  *plan = nullptr;
  int rc = validate(ncrms, nx, nz, ntracers);
  if (rc) return rc;
  const int var = var_in >= 0 ? var_in : variant();
  // wave-major: fp64, and fp32 with an even ncrms (two adjacent instances per lane = 8-byte elements) -- or, with the
  // switch of include/mpdata_hip.h 3f on, an odd one: one more pair, whose upper half is a phantom
  const bool pairs_ok = eb == 8 || (ncrms & 1) == 0 || f32_odd_ncrms();
  const bool wmaj = pairs_ok && wm_lps_for(nz) != 0 &&
                    plan_layout_default() == MPDATA_LAYOUT_WAVEMAJOR && tile_override() < 0;
  // windowed (include/mpdata_hip.h 3e): above the tallest wave-major form, when switched on, under the same conditions
  const bool windowed = tall_columns() && nz > MPDATA_WM_NZ_MAX && pairs_ok &&
                        plan_layout_default() == MPDATA_LAYOUT_WAVEMAJOR && tile_override() < 0;
  MpdataTileInfo t;
  if (!wmaj && !windowed) {
    rc = choose_tile(var, ncrms, nx, nz, &t, eb);
    if (rc) return rc;
  }
  mpdata_plan* p = (mpdata_plan*)calloc(1, sizeof(mpdata_plan));
  if (!p) return set_err(MPDATA_EINVAL, "out of host memory");
  p->ncrms = ncrms; p->nx = nx; p->nz = nz; p->ntracers = ntracers; p->eb = eb;
  p->variant = var;
  p->layout = (wmaj || windowed) ? MPDATA_LAYOUT_WAVEMAJOR : MPDATA_LAYOUT_REFERENCE;
  p->W = 1;
  p->sz = sizes_of(ncrms, nx, nz, ntracers);
  p->halo_ok = (unsigned char*)calloc((size_t)ntracers, 1);
  if (!p->halo_ok) {
    free(p);
    return set_err(MPDATA_EINVAL, "out of host memory");
  }
  hipError_t e = hipGetDevice(&p->device);
  if (e == hipSuccess && windowed) {
    int k0, nz_w, own0, own1;
    p->W = mpd_level_window(nz, 0, &k0, &nz_w, &own0, &own1);
    p->seam_ok = (unsigned char*)calloc((size_t)ntracers, 1);
    if (!p->seam_ok) rc = set_err(MPDATA_EINVAL, "out of host memory");
    if (!rc && ncrms > INT64_MAX / p->W) rc = set_err(MPDATA_EINVAL, "ncrms = %lld times %d level windows overflows", (long long)ncrms, p->W);
    if (!rc) rc = plan_create(ncrms * p->W, nx, nz_w, ntracers, &p->inner, eb, var);
    if (!rc && (p->inner->layout != MPDATA_LAYOUT_WAVEMAJOR || p->inner->slp != 1))
      rc = set_err(MPDATA_EINVAL, "internal: the windows of a tall plan are not one-instance tiles of a wave-major plan");
    if (rc) {
      mpdata_plan_destroy(p);
      return rc;
    }
    // the inner plan runs on this plan's stream, is timed by this plan's events and shares the halo bytes
    (void)hipStreamDestroy(p->inner->stream);
    p->inner->stream = nullptr; p->inner->own_stream = false; p->inner->timing = false;
    free(p->inner->halo_ok);
    p->inner->halo_ok = p->halo_ok;
    const size_t f1 = p->sz.f / ntracers;
    p->stage_elems = f1 > p->sz.w ? f1 : p->sz.w;
    e = hipMalloc(&p->flux_ref, p->sz.kz * ntracers * eb);
    if (e == hipSuccess) e = hipMemset(p->flux_ref, 0, p->sz.kz * ntracers * eb);
  }
  if (e == hipSuccess && !wmaj && !windowed) {
    const size_t nb[7] = {p->sz.f * eb, p->sz.u * eb, p->sz.w * eb, p->sz.k * eb, p->sz.kz * eb, p->sz.k * eb,
                          p->sz.kz * ntracers * eb};
    e = arena_alloc(p->arena, nb);
    if (e == hipSuccess) e = hipMemset(p->arena.p[6], 0, nb[6]);
    if (e == hipSuccess) {
      p->f = p->arena.p[0]; p->u = p->arena.p[1]; p->w = p->arena.p[2]; p->rho = p->arena.p[3];
      p->rhow = p->arena.p[4]; p->adz = p->arena.p[5]; p->flux = p->arena.p[6];
    }
  }
  if (e == hipSuccess && wmaj) {
    const int nzm = nz - 1;
    const int web = 8;   // bytes of an element on the wave-major side (fp32: a pair of instances)
    p->wm_ncrms = eb == 8 ? ncrms : (ncrms + 1) / 2;
    p->odd = eb == 4 && (ncrms & 1);
    p->lps = wm_lps_for(nz); p->slp = p->lps >= 64 ? 1 : 64 / p->lps; p->wpb = wm_wpb();
    p->ntiles = (int)((p->wm_ncrms + p->slp - 1) / p->slp);
    p->chunk = (long long)p->slp * nzm;
    p->main_e = p->chunk * web / 128 * (128 / web);
    // The counted waits of the wave-major kernels (s_waitcnt vmcnt(N), mpdata_kernel_wm_body.h) count
    // INSTRUCTIONS: every column-pair fetch of an array must issue exactly two -- the lanes of the
    // line-aligned main part in one, the other lanes in the second --, so both lane sets must be
    // non-empty: 128 <= main part <= 384 bytes.  True for every (LPS, nz) the kernels are built for
    // (chunk = (64/LPS) * nzm * 8 bytes with LPS/2 <= nzm < LPS, nz >= 3: 128 .. 504 bytes); checked
    // here so that a future tiling cannot break the wait silently.
    if (p->lps <= 64 && (p->main_e * web < 128 || p->main_e * web > 384)) {   // (nz > 64: one fetch instruction per array and pair)
      free(p->halo_ok);
      free(p);
      return set_err(MPDATA_EUNSUPPORTED, "internal: column chunk of %lld bytes breaks the two-instructions-per-fetch "
                                          "invariant of the wave-major kernels", (long long)(p->chunk * web));
    }
    {  // tiles start on 128-byte lines, an ODD number of lines apart (a power-of-two-ish stride
       // would put the same column of every tile on the same HBM channels: measured -5 %)
      long long lines = ((long long)(nx + 6) * p->chunk * web + 127) / 128;
      if ((lines & 1) == 0) ++lines;
      p->tile_elems = lines * (128 / web);
    }
    const size_t tile_arr = (size_t)p->ntiles * p->tile_elems * web;
    const size_t f1 = p->sz.f / ntracers;
    p->stage_elems = f1 > p->sz.w ? f1 : p->sz.w;
    if (e == hipSuccess) e = hipMalloc(&p->pf, tile_arr * ntracers);
    if (e == hipSuccess) e = hipMalloc(&p->pu, tile_arr);
    if (e == hipSuccess) e = hipMalloc(&p->pw, tile_arr);
    if (e == hipSuccess) e = hipMalloc(&p->pkc, (size_t)p->ntiles * 3 * p->chunk * web);
    if (e == hipSuccess) e = hipMalloc(&p->pflux, (size_t)p->ntiles * p->chunk * ntracers * web);
    if (e == hipSuccess) e = hipMalloc(&p->flux_ref, p->sz.kz * ntracers * eb);
    // EXACT: the park array of the limited vertical fluxes (bit-identical flux, see plan_flux_finish): [tracer][tile][nx][64]
    // 8-byte elements, the size of f's interior.  MPDATA_EXACT_FLUX=sum does without it (flux = upwind sum + limited sum,
    // <= 1e-13 relative, the behaviour up to round 3; a quarter faster in the EXACT variant).
    p->park_regs = var == MPDATA_VARIANT_EXACT && exact_flux_in_regs() && nx <= MPDATA_WM_NPK2;
    if (e == hipSuccess && var == MPDATA_VARIANT_EXACT && exact_flux_in_order() && !p->park_regs) {
      p->wpark_bytes = (size_t)ntracers * p->ntiles * wm_nkw_for(nz) * (size_t)nx * 64 * 8;
      e = hipMalloc(&p->wpark, p->wpark_bytes);
      if (e != hipSuccess) {
        (void)hipGetLastError();
        mpdata_plan_destroy(p);
        return set_err((int)e, "mpdata_plan_create (EXACT): no memory for the %.1f-GB park array of the bit-identical flux; "
                               "MPDATA_EXACT_FLUX=sum does without it (flux then equal to 1e-13 relative)", p->wpark_bytes / 1e9);
      }
    }
    // flux: level nz and tracers that are never run export what was imported -- or zeros
    if (e == hipSuccess) e = hipMemset(p->flux_ref, 0, p->sz.kz * ntracers * eb);
    if (e == hipSuccess) e = hipMemset(p->pflux, 0, (size_t)p->ntiles * p->chunk * ntracers * web);
    // u, w have column slots that nothing ever fills or fetches (c = 0; c = nx+5 of w)
    if (e == hipSuccess) e = hipMemset(p->pu, 0, tile_arr);
    if (e == hipSuccess) e = hipMemset(p->pw, 0, tile_arr);
  }
  if (e == hipSuccess) e = hipStreamCreate(&p->stream);
  if (e == hipSuccess) p->own_stream = true;
  if (e == hipSuccess) e = hipEventCreate(&p->ev0);
  if (e == hipSuccess) e = hipEventCreate(&p->ev1);
  p->timing = true;
  if (e != hipSuccess) {
    mpdata_plan_destroy(p);
    return hip_err(e, "mpdata_plan_create");
  }
  *plan = p;
  return 0;
}
int mpdata_plan_create(int64_t ncrms, int nx, int nz, int ntracers, mpdata_plan** plan) {
  return plan_create(ncrms, nx, nz, ntracers, plan, 8);
}
int mpdata_plan_create_f32(int64_t ncrms, int nx, int nz, int ntracers, mpdata_plan** plan) {
  return plan_create(ncrms, nx, nz, ntracers, plan, 4);
}

// flux of every tracer := 0 on the plan's stream (an upload without a flux array: level nz and tracers
// that are never run then download as zeros); also used by the multi-GPU upload on its per-GPU plans
extern "C++" int mpdata_plan_zero_flux_internal(mpdata_plan* p) {
  DevGuard g(p->device);
  void* fl = p->layout == MPDATA_LAYOUT_REFERENCE ? p->flux : p->flux_ref;
  HIP_TRY(hipMemsetAsync(fl, 0, p->sz.kz * p->ntracers * p->eb, p->stream));
  if (p->inner) return mpdata_plan_zero_flux_internal(win_inner(p));
  if (p->layout == MPDATA_LAYOUT_WAVEMAJOR)
    HIP_TRY(hipMemsetAsync(p->pflux, 0, (size_t)p->ntiles * p->chunk * p->ntracers * 8, p->stream));
  return 0;
}

static int plan_upload(mpdata_plan* p, const void* f, const void* u, const void* w, const void* rho,
                       const void* rhow, const void* adz, const void* flux, int eb) {
  int rc = plan_check(p, eb);
  if (rc) return rc;
  if (!f || !u || !w || !rho || !rhow || !adz) return set_err(MPDATA_EINVAL, "null array pointer");
  if (p->multi) {
    rc = mpdata_multi_upload(p->multi, f, u, w, rho, rhow, adz, flux);
    if (!rc) p->uploaded = true;
    return rc;
  }
  DevGuard g(p->device);
  // flux is intent(out) in the reference but its level nz is never written
  // (reference :541, :624 touch 1..nzm only): carry the caller's values over
  if (!flux) {
    rc = mpdata_plan_zero_flux_internal(p);
    if (rc) return rc;
  }
  rc = plan_import(p, f, u, w, rho, rhow, adz, flux, 0, p->ntracers, false);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(p->stream));
  p->uploaded = true;
  return 0;
}
int mpdata_plan_upload(mpdata_plan* p, const double* f, const double* u, const double* w,
                       const double* rho, const double* rhow, const double* adz,
                       const double* flux) {
  return plan_upload(p, f, u, w, rho, rhow, adz, flux, 8);
}
int mpdata_plan_upload_f32(mpdata_plan* p, const float* f, const float* u, const float* w,
                           const float* rho, const float* rhow, const float* adz,
                           const float* flux) {
  return plan_upload(p, f, u, w, rho, rhow, adz, flux, 4);
}

int mpdata_plan_import_device(mpdata_plan* p, const void* f, const void* u, const void* w, const void* rho,
                              const void* rhow, const void* adz, const void* flux, int first_tracer,
                              int ntracers) {
  if (!p) return set_err(MPDATA_EINVAL, "null plan");
  int rc = tracer_range(p, first_tracer, ntracers);
  if (rc) return rc;
  if (p->multi) {   // the arrays live on the ROOT GPU (shard 0's device), full width: scatter them (RCCL over xGMI)
    rc = mpdata_multi_scatter_device(p->multi, f, u, w, rho, rhow, adz, flux, first_tracer, ntracers);
    if (!rc) {
      p->uploaded = true;
      for (int g = 0; g < mpdata_multi_ngpus(p->multi); ++g) mpdata_multi_sub(p->multi, g)->uploaded = true;
    }
    return rc;
  }
  DevGuard g(p->device);
  rc = plan_import(p, f, u, w, rho, rhow, adz, flux, first_tracer, ntracers, true);
  if (rc) return rc;
  p->uploaded = true;  // (the caller is responsible for having provided every array once)
  return 0;
}

int mpdata_plan_export_device(mpdata_plan* p, void* f, void* flux, int first_tracer, int ntracers) {
  if (!p) return set_err(MPDATA_EINVAL, "null plan");
  int rc = tracer_range(p, first_tracer, ntracers);
  if (rc) return rc;
  if (p->multi) {   // gather to arrays on the root GPU
    for (int g = 0; g < mpdata_multi_ngpus(p->multi); ++g)
      if (!mpdata_multi_sub(p->multi, g)->uploaded) return set_err(MPDATA_ESTATE, "mpdata_plan_export_device before upload / import (shard %d)", g);
    return mpdata_multi_gather_device(p->multi, f, flux, first_tracer, ntracers);
  }
  if (!p->uploaded) return set_err(MPDATA_ESTATE, "mpdata_plan_export_device before upload / import");
  DevGuard g(p->device);
  return plan_export(p, f, flux, first_tracer, ntracers, true);
}

// ---- 3d: blocks of instances
int mpdata_plan_import_instances_device(mpdata_plan* p, int64_t sl0, int64_t n, const void* f, const void* u, const void* w,
                                        const void* rho, const void* rhow, const void* adz, const void* flux, int first_tracer,
                                        int ntracers) {
  int rc = block_range("mpdata_plan_import_instances_device", p, sl0, n);
  if (rc) return rc;
  rc = tracer_range(p, first_tracer, ntracers);
  if (rc) return rc;
  if (!f && !u && !w && !rho && !rhow && !adz && !flux)
    return set_err(MPDATA_EINVAL, "mpdata_plan_import_instances_device: all seven array pointers are NULL");
  if (!p->uploaded)
    return set_err(MPDATA_ESTATE, "mpdata_plan_import_instances_device before the plan was filled once (upload / whole import): "
                                  "a plan is not first filled block by block");
  if ((u && !p->have_u) || (w && !p->have_w))
    return set_err(MPDATA_ESTATE, "mpdata_plan_import_instances_device: a block of %s while the plan holds no velocities (none "
                                  "imported yet, or mpdata_plan_run_uw ran since): import whole u and w first",
                   (u && !p->have_u) ? "u" : "w");
  DevGuard g(p->device);
  return plan_import_block(p, sl0, n, f, u, w, rho, rhow, adz, flux, first_tracer, ntracers);
}

int mpdata_plan_export_instances_device(mpdata_plan* p, int64_t sl0, int64_t n, void* f, void* flux, int first_tracer, int ntracers) {
  int rc = block_range("mpdata_plan_export_instances_device", p, sl0, n);
  if (rc) return rc;
  rc = tracer_range(p, first_tracer, ntracers);
  if (rc) return rc;
  if (!f && !flux) return set_err(MPDATA_EINVAL, "mpdata_plan_export_instances_device: f and flux are both NULL");
  if (!p->uploaded) return set_err(MPDATA_ESTATE, "mpdata_plan_export_instances_device before upload / import");
  DevGuard g(p->device);
  return plan_export_block(p, sl0, n, f, flux, first_tracer, ntracers);
}

// host arrays, all tracers, synchronous: the block goes through a device staging buffer of its own size
static int plan_download_block(mpdata_plan* p, int64_t sl0, int64_t n, void* f, void* flux, int eb) {
  int rc = block_range("mpdata_plan_download_instances", p, sl0, n);
  if (rc) return rc;
  if (!f && !flux) return set_err(MPDATA_EINVAL, "mpdata_plan_download_instances: f and flux are both NULL");
  rc = plan_check(p, eb);
  if (rc) return rc;
  if (!p->uploaded) return set_err(MPDATA_ESTATE, "mpdata_plan_download_instances before upload / import");
  DevGuard g(p->device);
  const size_t fb = f ? (size_t)n * (p->nx + 6) * (p->nz - 1) * p->ntracers * eb : 0;
  const size_t lb = flux ? (size_t)n * p->nz * p->ntracers * eb : 0;
  rc = plan_bstage(p, fb + lb);
  if (rc) return rc;
  void* df = f ? p->bstage : nullptr;
  void* dl = flux ? (char*)p->bstage + fb : nullptr;
  rc = plan_export_block(p, sl0, n, df, dl, 0, p->ntracers);
  if (rc) return rc;
  if (f) HIP_TRY(hipMemcpyAsync(f, df, fb, hipMemcpyDeviceToHost, p->stream));
  if (flux) HIP_TRY(hipMemcpyAsync(flux, dl, lb, hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  return 0;
}
int mpdata_plan_download_instances(mpdata_plan* p, int64_t sl0, int64_t n, double* f, double* flux) {
  return plan_download_block(p, sl0, n, f, flux, 8);
}
int mpdata_plan_download_instances_f32(mpdata_plan* p, int64_t sl0, int64_t n, float* f, float* flux) {
  return plan_download_block(p, sl0, n, f, flux, 4);
}

// (EXACT wave-major runs: the finishing kernel of the bit-identical flux, behind the plan kernels on the same stream)
static int plan_flux_finish(mpdata_plan* p, const MpdataWmArgs& a, int count) {
  if (!a.wpark) return 0;
  const long long waves = (long long)count * p->ntiles * a.nkw;
  const unsigned blocks = (unsigned)((waves + 3) / 4);
  if (p->eb == 8)
    hipLaunchKernelGGL(flux_finish_kernel<double>, dim3(blocks), dim3(256), 0, p->stream, a.flux, (const double*)a.wpark, p->ntiles,
                       p->nx, p->nz - 1, p->lps, a.flux_tstride, count, a.nkw);
  else
    hipLaunchKernelGGL(flux_finish_kernel<float2>, dim3(blocks), dim3(256), 0, p->stream, (float2*)a.flux, (const float2*)a.wpark,
                       p->ntiles, p->nx, p->nz - 1, p->lps, a.flux_tstride, count, a.nkw);
  HIP_TRY(hipGetLastError());
  return 0;
}

// (uw_conv: that kernel also writes the velocities into the plan's own u, w)
static int plan_launch(mpdata_plan* p, int first, int count, const void* u_ref = nullptr, const void* w_ref = nullptr,
                       bool uw_conv = false) {
  int rc = 0;
  if (p->inner) {   // windowed: the plan kernel on the windows; it leaves the margin levels of every seam wrong
    if (u_ref) return set_err(MPDATA_EINVAL, "internal: a windowed plan takes u, w through the split");
    memset(p->seam_ok + first, 0, (size_t)count);
    return plan_launch(win_inner(p), first, count);
  }
  if (p->layout == MPDATA_LAYOUT_WAVEMAJOR) {
    MpdataWmArgs a;
    a.f = (double*)p->pf + (long long)first * p->ntiles * p->tile_elems;
    a.u = (const double*)p->pu; a.w = (const double*)p->pw; a.kc = (const double*)p->pkc;
    a.flux = (double*)p->pflux + (long long)first * p->ntiles * p->chunk;
    a.ntiles = p->ntiles; a.nx = p->nx; a.nz = p->nz; a.ntracers = count;
    a.tile_elems = p->tile_elems;
    a.f_tstride = (long long)p->ntiles * p->tile_elems;
    a.flux_tstride = (long long)p->ntiles * p->chunk;
    a.reverse = serpentine() ? (int)(p->runs++ & 1u) : 0;
    a.u_ref = (const double*)u_ref; a.w_ref = (const double*)w_ref; a.ncrms = p->ncrms;
    a.dbg = debug_buffer();   // (null unless a diagnostic build was handed a stamp buffer)
    // EXACT plans: the park array of the limited vertical fluxes (bit-identical flux; allocated with the plan)
    a.park_regs = (p->park_regs && !u_ref) ? 1 : 0;
    a.nkw = wm_nkw_for(p->nz);
    if (u_ref && p->park_regs && !p->wpark) {
      // the kernel that reads u, w from the reference layout has no register-park form (its EXACT build takes every
      // register it can get): the park array after all, allocated by the first such call
      p->wpark_bytes = (size_t)p->ntracers * p->ntiles * wm_nkw_for(p->nz) * (size_t)p->nx * 64 * 8;
      const hipError_t e = hipMalloc(&p->wpark, p->wpark_bytes);
      if (e != hipSuccess) {
        (void)hipGetLastError();
        p->wpark = nullptr;
        return set_err((int)e, "mpdata_plan_run_uw (EXACT): no memory for the %.1f-GB park array of the bit-identical flux; "
                               "MPDATA_EXACT_FLUX=sum does without it", p->wpark_bytes / 1e9);
      }
    }
    a.wpark = (p->wpark && !a.park_regs) ? (double*)p->wpark + (long long)first * p->ntiles * a.nkw * ((long long)p->nx * 64) : nullptr;
    a.lwt = (a.wpark || u_ref) ? 0 : wm_lwt_for(p->nz);   // (the park array is laid out for whole-wave windows)
    const bool fast = p->variant == MPDATA_VARIANT_FAST;
    if (u_ref) {
      a.reverse = 0;
      const bool okx = fast ? mpdata_fast::launch_wm_uw(p->lps, a, (void*)p->stream, uw_conv)
                            : mpdata_exact::launch_wm_uw(p->lps, a, (void*)p->stream, uw_conv);
      if (!okx) return set_err(MPDATA_EINVAL, "wave-major u,w-reference kernel LPS=%d not instantiated", p->lps);
      HIP_TRY(hipGetLastError());
      return plan_flux_finish(p, a, count);
    }
    const int fl = wm_flags();
    const bool ok = p->eb == 8 ? (fast ? mpdata_fast::launch_wm(p->lps, p->wpb, a, (void*)p->stream, fl)
                                       : mpdata_exact::launch_wm(p->lps, p->wpb, a, (void*)p->stream, fl))
                               : (fast ? mpdata_fast::launch_wm_f32(p->lps, p->wpb, a, (void*)p->stream, fl)
                                       : mpdata_exact::launch_wm_f32(p->lps, p->wpb, a, (void*)p->stream, fl));
    if (!ok) return set_err(MPDATA_EINVAL, "wave-major kernel LPS=%d WPB=%d not instantiated", p->lps, p->wpb);
    HIP_TRY(hipGetLastError());
    rc = plan_flux_finish(p, a, count);
    if (rc) return rc;
  } else {
    const size_t f1 = p->sz.f / p->ntracers;
    // (the plan's own variant, passed explicitly: the global one may be changed by other threads)
    if (p->eb == 8)
      rc = advect_device<double>(p->ncrms, p->nx, p->nz, count, (double*)p->f + first * f1, (const double*)p->u,
                                 (const double*)p->w, (const double*)p->rho, (const double*)p->rhow,
                                 (const double*)p->adz, (double*)p->flux + first * p->sz.kz, (void*)p->stream, p->variant);
    else
      rc = advect_device<float>(p->ncrms, p->nx, p->nz, count, (float*)p->f + first * f1, (const float*)p->u,
                                (const float*)p->w, (const float*)p->rho, (const float*)p->rhow,
                                (const float*)p->adz, (float*)p->flux + first * p->sz.kz, (void*)p->stream, p->variant);
    if (rc) return rc;
  }
  return 0;
}
int mpdata_plan_run_tracers(mpdata_plan* p, int first, int count) {
  if (!p) return set_err(MPDATA_EINVAL, "null plan");
  int rc = tracer_range(p, first, count);
  if (rc) return rc;
  if (p->multi) {   // (the per-GPU plans check their own state: they may have been filled directly)
    rc = mpdata_multi_run(p->multi, first, count);
    if (!rc) p->ran = true;
    return rc;
  }
  if (!p->uploaded) return set_err(MPDATA_ESTATE, "mpdata_plan_run before mpdata_plan_upload");
  if (!p->have_u || !p->have_w)
    return set_err(MPDATA_ESTATE, "mpdata_plan_run: the plan holds no velocities (none imported yet, or mpdata_plan_run_uw "
                                  "ran since -- it leaves none behind): import u and w first");
  DevGuard g(p->device);
  if (p->timing) HIP_TRY(hipEventRecord(p->ev0, p->stream));
  rc = plan_seams(p, first, count);   // (windowed plans; in front of the wrap: the two commute, the order is fixed)
  if (!rc) rc = plan_wrap_f(p, first, count);
  memset(p->halo_ok + first, 0, (size_t)count);   // (the run leaves first-pass values in the halos)
  if (!rc) rc = plan_launch(p, first, count);
  if (rc) return rc;
  if (p->timing) HIP_TRY(hipEventRecord(p->ev1, p->stream));
  p->ran = p->timing;
  return 0;
}
int mpdata_plan_run(mpdata_plan* p) {
  if (!p) return set_err(MPDATA_EINVAL, "null plan");
  return mpdata_plan_run_tracers(p, 0, p->ntracers);
}

// One step on FRESH velocities: u, w are reference-layout device arrays (what a CRM whose state
// lives on the device hands over every step, reference :107 `update device` then kernels), f stays
// in the plan.  The layout entry of u, w is part of the call (and of its event time).
int mpdata_plan_run_uw(mpdata_plan* p, int first, int count, const void* u, const void* w) {
  if (!p) return set_err(MPDATA_EINVAL, "null plan");
  if (!u || !w) return set_err(MPDATA_EINVAL, "null array pointer");
  int rc = tracer_range(p, first, count);
  if (rc) return rc;
  if (p->multi) {   // u, w: full-width arrays on the root GPU -- scatter them (RCCL over xGMI), then every GPU runs
    for (int g = 0; g < mpdata_multi_ngpus(p->multi); ++g)
      if (!mpdata_multi_sub(p->multi, g)->uploaded) return set_err(MPDATA_ESTATE, "mpdata_plan_run_uw before upload / import (shard %d)", g);
    rc = mpdata_multi_scatter_device(p->multi, nullptr, u, w, nullptr, nullptr, nullptr, nullptr, 0, 0);
    if (!rc) rc = mpdata_multi_run(p->multi, first, count);
    // the same post-condition as on one GPU: no velocities are left behind
    for (int g = 0; g < mpdata_multi_ngpus(p->multi); ++g) {
      mpdata_plan* q = mpdata_multi_sub(p->multi, g);
      q->have_u = q->have_w = false;
    }
    if (!rc) p->ran = true;
    return rc;
  }
  if (!p->uploaded) return set_err(MPDATA_ESTATE, "mpdata_plan_run_uw before upload / import");
  DevGuard g(p->device);
  if (p->timing) HIP_TRY(hipEventRecord(p->ev0, p->stream));
  // one fp64 tracer of a wave-major plan: the kernel fetches u, w from the caller's arrays itself
  // (16-byte row pieces: even ncrms, 16-byte aligned bases; 32-bit offsets: arrays below 4 GiB);
  // MPDATA_RUN_UW=import forces the conversion path (tests, A/B)
  static const bool force_import = getenv("MPDATA_RUN_UW") && !strcmp(getenv("MPDATA_RUN_UW"), "import");
  const bool ring = p->layout == MPDATA_LAYOUT_WAVEMAJOR && !p->inner && p->eb == 8 && (p->ncrms & 1) == 0 && p->lps <= 64 &&
                    (((uintptr_t)u | (uintptr_t)w) & 15) == 0 &&
                    (double)p->ncrms * (p->nx + 5) * p->nz * 8.0 < 4294967000.0 && !force_import;
  // POST-CONDITION, the same on every path (which one runs depends on alignment, parity of ncrms, nz,
  // the tracer count ...): the plan holds NO velocities afterwards.  The one-tracer kernel never writes the
  // plan's u, w (they would be stale), the other paths overwrite them (they would be the new ones):
  // neither is promised, mpdata_plan_run returns MPDATA_ESTATE until u, w are imported again.
  p->have_u = p->have_w = false;
  rc = plan_seams(p, first, count);
  if (!rc) rc = plan_wrap_f(p, first, count);
  if (rc) return rc;
  memset(p->halo_ok + first, 0, (size_t)count);
  if (ring && count == 1) {
    rc = plan_launch(p, first, count, u, w);
  } else if (ring && p->lps <= 32) {
    // a tracer batch: its FIRST tracer goes through the kernel that reads the caller's u, w -- in the form
    // that also writes them into the plan's arrays as it goes --, the others through the batch kernel behind
    // it: no conversion pass (0.54 ms at ncrms = 65536) in front of the batch
    rc = plan_launch(p, first, 1, u, w, true);
    if (!rc) rc = plan_launch(p, first + 1, count - 1);
  } else {
    rc = plan_import(p, nullptr, u, w, nullptr, nullptr, nullptr, nullptr, 0, 1, true);
    if (!rc) rc = plan_launch(p, first, count);
    p->have_u = p->have_w = false;
  }
  if (rc) return rc;
  if (p->timing) HIP_TRY(hipEventRecord(p->ev1, p->stream));
  p->ran = p->timing;
  return 0;
}

int mpdata_plan_sync(mpdata_plan* p) {
  if (!p) return set_err(MPDATA_EINVAL, "null plan");
  if (p->multi) return mpdata_multi_sync(p->multi);
  DevGuard g(p->device);
  HIP_TRY(hipStreamSynchronize(p->stream));
  return 0;
}

static int plan_download(mpdata_plan* p, void* f, void* flux, int eb) {
  int rc = plan_check(p, eb);
  if (rc) return rc;
  if (p->multi) {   // (the shards may have been filled directly: mpdata_plan_shard_plan + import)
    for (int g = 0; g < mpdata_multi_ngpus(p->multi); ++g)
      if (!mpdata_multi_sub(p->multi, g)->uploaded) return set_err(MPDATA_ESTATE, "mpdata_plan_download before upload (shard %d)", g);
    return mpdata_multi_download(p->multi, f, flux);
  }
  if (!p->uploaded) return set_err(MPDATA_ESTATE, "mpdata_plan_download before upload");
  DevGuard g(p->device);
  rc = plan_export(p, f, flux, 0, p->ntracers, false);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(p->stream));
  return 0;
}
int mpdata_plan_download(mpdata_plan* p, double* f, double* flux) { return plan_download(p, f, flux, 8); }
int mpdata_plan_download_f32(mpdata_plan* p, float* f, float* flux) { return plan_download(p, f, flux, 4); }

int mpdata_plan_last_kernel_ms(mpdata_plan* p, double* ms) {
  if (!p || !ms) return set_err(MPDATA_EINVAL, "null argument");
  if (!p->ran) return set_err(MPDATA_ESTATE, "no run recorded");
  if (p->multi) return mpdata_multi_last_kernel_ms(p->multi, ms);
  DevGuard g(p->device);
  HIP_TRY(hipEventSynchronize(p->ev1));
  float t = 0.f;
  HIP_TRY(hipEventElapsedTime(&t, p->ev0, p->ev1));
  *ms = t;
  return 0;
}

int mpdata_plan_set_stream(mpdata_plan* p, void* stream) {
  if (!p) return set_err(MPDATA_EINVAL, "null plan");
  if (p->multi) return set_err(MPDATA_EUNSUPPORTED, "a multi-GPU plan runs on its own streams, one per device");
  DevGuard g(p->device);
  HIP_TRY(hipStreamSynchronize(p->stream));
  if (p->own_stream) (void)hipStreamDestroy(p->stream);
  p->stream = (hipStream_t)stream;
  p->own_stream = false;
  return 0;
}
// The event pair a plan records around every run costs two marker packets between consecutive
// launches of a stream (about 1.5 % of a 0.4-ms kernel): a caller that times a whole loop itself
// switches it off (mpdata_plan_last_kernel_ms then reports MPDATA_ESTATE).
int mpdata_plan_set_timing(mpdata_plan* p, int on) {
  if (!p) return set_err(MPDATA_EINVAL, "null plan");
  // (switched off, the last recorded pair is forgotten: mpdata_plan_last_kernel_ms is a state error from this call on,
  //  not only from the next run on, until a run has been recorded with the pair on again)
  if (p->multi) {
    for (int g = 0; g < mpdata_multi_ngpus(p->multi); ++g) {
      mpdata_plan* q = mpdata_multi_sub(p->multi, g);
      q->timing = on != 0;
      if (!on) q->ran = false;
    }
    if (!on) p->ran = false;
    return 0;
  }
  p->timing = on != 0;
  if (!on) p->ran = false;
  return 0;
}
int mpdata_plan_layout(const mpdata_plan* p) { return p ? p->layout : MPDATA_EINVAL; }
// level windows (include/mpdata_hip.h 3e)
int mpdata_plan_level_windows(const mpdata_plan* p) {
  if (!p) return MPDATA_EINVAL;
  if (p->multi) return mpdata_plan_level_windows(mpdata_multi_sub(p->multi, 0));
  return p->inner ? p->W : 1;
}
int mpdata_level_window(int nz, int h, int* k0, int* nz_w, int* own0, int* own1) {
  int a = 0, b = 0, c = 0, d = 0;
  const int W = mpd_level_window(nz, h, &a, &b, &c, &d);
  if (W < 1) return set_err(MPDATA_EINVAL, "mpdata_level_window: nz = %d, window %d", nz, h);
  if (k0) *k0 = a;
  if (nz_w) *nz_w = b;
  if (own0) *own0 = c;
  if (own1) *own1 = d;
  return W;
}
int mpdata_plan_device(const mpdata_plan* p) { return p ? p->device : MPDATA_EINVAL; }

// Lateral boundary mode.  PERIODIC: f's halo columns are refreshed from the interior in front of every run and every
// read-back (plan_wrap_f).  Back to GIVEN: the plan first holds what an export would return (wrapped halos).
int mpdata_plan_set_boundary(mpdata_plan* p, int mode) {
  if (!p) return set_err(MPDATA_EINVAL, "null plan");
  if (mode != MPDATA_BOUNDARY_GIVEN && mode != MPDATA_BOUNDARY_PERIODIC) return set_err(MPDATA_EINVAL, "unknown boundary mode %d", mode);
  if (p->multi) {   // every shard plan holds its own halos
    for (int g = 0; g < mpdata_multi_ngpus(p->multi); ++g) {
      const int rc = mpdata_plan_set_boundary(mpdata_multi_sub(p->multi, g), mode);
      if (rc) return rc;
    }
    p->boundary = mode;
    return 0;
  }
  if (p->boundary == MPDATA_BOUNDARY_PERIODIC && mode == MPDATA_BOUNDARY_GIVEN && p->uploaded) {
    DevGuard g(p->device);
    const int rc = plan_wrap_f(p, 0, p->ntracers);
    if (rc) return rc;
  }
  p->boundary = mode;
  return 0;
}
int mpdata_plan_boundary(const mpdata_plan* p) { return p ? p->boundary : MPDATA_EINVAL; }

// Reference-layout device arrays made periodic in x, in place (include/mpdata_hip.h 3c).
static int periodic_halo(int64_t ncrms, int nx, int nz, int ntracers, void* f, void* u, void* w, void* stream, int eb) {
  int rc = validate(ncrms, nx, nz, ntracers);
  if (rc) return rc;
  if (!f && !u && !w) return set_err(MPDATA_EINVAL, "mpdata_periodic_halo_device: f, u and w are all NULL");
  const hipStream_t s = (hipStream_t)stream;
  const int nzm = nz - 1;
  if (f) HIP_TRY(mpdata_layout_periodic_halo_ref(f, eb, ncrms, nx, nx + 6, 2, nzm, ntracers, -2, nx + 3, s));
  if (u) HIP_TRY(mpdata_layout_periodic_halo_ref(u, eb, ncrms, nx, nx + 5, 1, nzm, 1, -1, nx + 3, s));
  if (w) HIP_TRY(mpdata_layout_periodic_halo_ref(w, eb, ncrms, nx, nx + 4, 1, nz, 1, -1, nx + 2, s));
  return 0;
}
int mpdata_periodic_halo_device(int64_t ncrms, int nx, int nz, int ntracers, double* f, double* u, double* w, void* stream) {
  return periodic_halo(ncrms, nx, nz, ntracers, f, u, w, stream, 8);
}
int mpdata_periodic_halo_f32_device(int64_t ncrms, int nx, int nz, int ntracers, float* f, float* u, float* w, void* stream) {
  return periodic_halo(ncrms, nx, nz, ntracers, f, u, w, stream, 4);
}

// ---- multi-GPU plans (mpdata_multi.hip): the same handle type; upload / run / run_tracers /
// sync / download / last_kernel_ms / destroy dispatch to the per-device plans.
static int plan_create_multi(int64_t ncrms, int nx, int nz, int ntracers, int ngpus, const int* devices,
                             mpdata_plan** plan, int eb) {
  if (!plan) return set_err(MPDATA_EINVAL, "null plan pointer");
  *plan = nullptr;
  int rc = validate(ncrms, nx, nz, ntracers);
  if (rc) return rc;
  mpdata_plan* p = (mpdata_plan*)calloc(1, sizeof(mpdata_plan));
  if (!p) return set_err(MPDATA_EINVAL, "out of host memory");
  p->ncrms = ncrms; p->nx = nx; p->nz = nz; p->ntracers = ntracers; p->eb = eb;
  p->variant = variant(); p->device = -1; p->layout = -1;
  p->sz = sizes_of(ncrms, nx, nz, ntracers);
  rc = mpdata_multi_create(ncrms, nx, nz, ntracers, ngpus, devices, eb, &p->multi);
  if (rc) { free(p); return rc; }
  *plan = p;
  return 0;
}
int mpdata_plan_create_multi(int64_t ncrms, int nx, int nz, int ntracers, int ngpus, mpdata_plan** plan) {
  // MPDATA_MULTI_DEVICES="0,0,1": explicit device list (tests on a one-GPU box repeat a device)
  const char* e = getenv("MPDATA_MULTI_DEVICES");
  if (e && *e) {
    int devs[64], n = 0;
    for (const char* q = e; *q && n < 64;) {
      devs[n++] = atoi(q);
      while (*q && *q != ',') ++q;
      if (*q == ',') ++q;
    }
    if (n >= ngpus) return plan_create_multi(ncrms, nx, nz, ntracers, ngpus, devs, plan, 8);
  }
  return plan_create_multi(ncrms, nx, nz, ntracers, ngpus, nullptr, plan, 8);
}
int mpdata_plan_create_multi_devices(int64_t ncrms, int nx, int nz, int ntracers, int ngpus, const int* devices,
                                     mpdata_plan** plan) {
  return plan_create_multi(ncrms, nx, nz, ntracers, ngpus, devices, plan, 8);
}
int mpdata_plan_ranks_seen(const mpdata_plan* p) {
  if (!p) return MPDATA_EINVAL;
  return p->multi ? mpdata_multi_ranks_seen(p->multi) : 0;
}
int mpdata_plan_ngpus(const mpdata_plan* p) { return !p ? MPDATA_EINVAL : (p->multi ? mpdata_multi_ngpus(p->multi) : 1); }
int mpdata_plan_shard(const mpdata_plan* p, int g, int* device, int64_t* sl0, int64_t* nloc) {
  if (!p) return set_err(MPDATA_EINVAL, "null plan");
  if (p->multi) return mpdata_multi_info(p->multi, g, device, sl0, nloc);
  if (g != 0) return set_err(MPDATA_EINVAL, "shard %d of a single-GPU plan", g);
  if (device) *device = p->device;
  if (sl0) *sl0 = 0;
  if (nloc) *nloc = p->ncrms;
  return 0;
}
mpdata_plan* mpdata_plan_shard_plan(mpdata_plan* p, int g) {
  if (!p) return nullptr;
  if (p->multi) return mpdata_multi_sub(p->multi, g);
  return g == 0 ? p : nullptr;
}
int mpdata_plan_transfer_stats(const mpdata_plan* p, double* scatter_s, double* gather_s, int64_t* scatter_bytes_per_peer,
                               int64_t* gather_bytes_per_peer, int* transport) {
  if (!p || !p->multi) return set_err(MPDATA_EINVAL, "not a multi-GPU plan");
  mpdata_multi_stats(p->multi, scatter_s, gather_s, scatter_bytes_per_peer, gather_bytes_per_peer, transport);
  return 0;
}

int mpdata_plan_destroy(mpdata_plan* p) {
  if (!p) return 0;
  if (p->inner) {   // (shares halo_ok and the stream)
    if (p->inner->halo_ok == p->halo_ok) p->inner->halo_ok = nullptr;
    if (!p->inner->own_stream) p->inner->stream = nullptr;
    mpdata_plan_destroy(p->inner);
  }
  free(p->halo_ok);
  free(p->seam_ok);
  if (p->multi) {
    const int rc = mpdata_multi_destroy(p->multi);
    free(p);
    return rc;
  }
  DevGuard g(p->device);
  arena_free(p->arena);
  void* bufs[10] = {p->pf, p->pu, p->pw, p->pkc, p->pflux, p->stage, p->flux_ref, p->wpark, p->bstage, p->dbuf};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  if (p->ev0) (void)hipEventDestroy(p->ev0);
  if (p->ev1) (void)hipEventDestroy(p->ev1);
  if (p->stream && p->own_stream) (void)hipStreamDestroy(p->stream);
  free(p);
  return 0;
}

// ---- calls on reference-layout device arrays with 65 <= nz <= 238 (round 5).  No x-marching kernel holds such an
//      instance in a wave and the k-marching fall-back runs at 13-16 Gcu/s (fp64, nx <= 140 only; fp32: nothing).  Such
//      a call goes through a wave-major plan kept per host thread instead: import f, u, w, rho, rhow, adz, flux
//      (the layout kernels), the plan kernel (several waves per instance), export f and flux -- everything on the
//      caller's stream, asynchronous as the direct call is, same results (EXACT bit-identical incl. flux; flux(:,nz)
//      carried through).  Costs the plan's memory (as much again as the call's arrays) until
//      mpdata_release_host_buffers() or the end of the thread; MPDATA_DEVICE_CALL=direct keeps the k-marching kernel.
namespace {
struct StagedPlan {
  mpdata_plan* p = nullptr;
  int var = -1;
  void release() {
    if (!p) return;
    int cur = 0;
    if (hipGetDevice(&cur) == hipSuccess) mpdata_plan_destroy(p);   // (else the runtime is gone: process exit)
    p = nullptr;
  }
  ~StagedPlan() { release(); }
};
thread_local StagedPlan t_staged;
}  // namespace
extern "C++" void mpd::staged_plan_release() { t_staged.release(); }
extern "C++" bool mpd::staged_call_applies(int64_t ncrms, int nz, int eb) {
  static const bool direct = getenv("MPDATA_DEVICE_CALL") && !strcmp(getenv("MPDATA_DEVICE_CALL"), "direct");
  // (3f: fp32 with an odd ncrms has no direct kernel above 32 levels -- from 33 on through the plan, when switched on)
  const bool odd = eb == 4 && (ncrms & 1);
  return !direct && nz > (odd ? 32 : 64) && (wm_lps_for(nz) != 0 || tall_columns()) && (!odd || f32_odd_ncrms()) &&
         plan_layout_default() == MPDATA_LAYOUT_WAVEMAJOR && tile_override() < 0;
}
extern "C++" int mpd::staged_device_call(int eb, int64_t ncrms, int nx, int nz, int ntracers, void* f, const void* u, const void* w,
                                         const void* rho, const void* rhow, const void* adz, void* flux, void* stream, int var) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  mpdata_plan* p = t_staged.p;
  if (p && !(p->ncrms == ncrms && p->nx == nx && p->nz == nz && p->ntracers == ntracers && p->eb == eb && p->variant == var &&
             p->device == dev)) {
    t_staged.release();
    p = nullptr;
  }
  if (!p) {
    const int rc = plan_create(ncrms, nx, nz, ntracers, &p, eb, var);
    if (rc) return rc;
    if (p->layout != MPDATA_LAYOUT_WAVEMAJOR) {   // (staged_call_applies and plan_create disagree: a bug, not a fall-back)
      mpdata_plan_destroy(p);
      return set_err(MPDATA_EINVAL, "internal: staged device call without a wave-major plan");
    }
    (void)hipStreamDestroy(p->stream);
    p->stream = (hipStream_t)stream;
    p->own_stream = false;
    p->timing = false;
    t_staged.p = p;
  }
  if (p->stream != (hipStream_t)stream) {   // the previous call's work may still use the plan's arrays
    HIP_TRY(hipStreamSynchronize(p->stream));
    p->stream = (hipStream_t)stream;
  }
  int rc = plan_import(p, f, u, w, rho, rhow, adz, flux, 0, ntracers, true);
  if (rc) return rc;
  p->uploaded = true;
  rc = plan_launch(p, 0, ntracers);
  if (rc) return rc;
  return plan_export(p, f, flux, 0, ntracers, true);
}

// ... on the device a plan's full-width arrays must live on: the plan's own device, the ROOT GPU
// (shard 0's device) of a multi-GPU plan
int mpdata_plan_device_alloc(mpdata_plan* plan, void** p, int64_t bytes) {
  if (!plan) return set_err(MPDATA_EINVAL, "null plan");
  int dev = plan->device;
  if (plan->multi) {
    const int rc = mpdata_multi_info(plan->multi, 0, &dev, nullptr, nullptr);
    if (rc) return rc;
  }
  DevGuard g(dev);
  return mpdata_device_alloc(p, bytes);
}
}  // extern "C"
