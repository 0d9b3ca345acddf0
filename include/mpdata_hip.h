/*
 * mpdata_hip.h -- C-ABI of libmpdata_hip.so: the MI355X (gfx950) replacement
 * for the compute body of the E3SM-MMF 2D MPDATA tracer-advection routine.
 *
 * What it replaces in the reference (E3SM-Project/codesign-kernels):
 *   mmf-mpdata-tracer/advect_scalar2D_pushncols_openacc.F90
 *     :72-244   subroutine advect_scalar2D_openacc_2   (8 OpenACC kernels)
 *     :247-474  subroutine advect_scalar2D_openacc_1   (17 OpenACC kernels)
 *   both of which compute what :477-642 advect_scalar2D_cpu computes, and
 *   mmf-mpdata-tracer/Makefile:17-20 (the `pgiacc` accelerator target).
 *
 * Array contract (identical to the reference's dummy arguments, :479-484, and
 * the host-associated global adz, :30).  Fortran column-major, the CRM
 * instance index `sl` (reference: nslices; here: ncrms) FASTEST, fp64:
 *   f   (ncrms, -2:nx+3, 1, nzm [, ntracers])  inout
 *   u   (ncrms, -1:nx+3, 1, nzm)               in
 *   w   (ncrms, -1:nx+2, 1, nz )               in   (level nz never read)
 *   rho (ncrms, nzm)  rhow(ncrms, nz)  adz(ncrms, nzm)   in
 *   flux(ncrms, nz [, ntracers])               out  (levels 1..nzm written;
 *                                                    level nz left untouched,
 *                                                    as the reference does)
 * with nzm = nz-1.  On return f holds: interior columns 1..nx = the advected
 * field; halo columns -1,0,nx+1,nx+2 = the first-pass (upwind) value;
 * columns -2 and nx+3 unchanged -- exactly the reference's in-place result.
 * `ntracers` > 1 is this library's extension: the same u,w,rho,rhow,adz
 * applied to ntracers fields, tracer index slowest.
 *
 * All functions return 0 on success, a negative MPDATA_E* code on argument
 * errors, or a positive hipError_t value; mpdata_last_error() gives text.
 * Nothing here falls back to a CPU path: without a usable HIP device the
 * calls fail.
 */
#ifndef MPDATA_HIP_H
#define MPDATA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPDATA_EINVAL (-1)      /* bad sizes / null pointer */
#define MPDATA_EUNSUPPORTED (-2) /* shape outside what the kernels cover */
#define MPDATA_ESTATE (-3)      /* plan used before upload, etc. */
#define MPDATA_ECOMM (-4)       /* RCCL error (multi-GPU plans) */

/* kernel variants (mpdata_set_variant / MPDATA_VARIANT env): */
#define MPDATA_VARIANT_EXACT 0  /* no FMA contraction, IEEE divide, the reference's
                                   expression order: f (every element, halos
                                   included) AND flux(:,1:nzm) are BIT-IDENTICAL
                                   to the reference CPU routine built with
                                   -ffp-contract=off.  For flux the kernels keep
                                   the nx limited vertical fluxes of every lane
                                   and add them onto the FINISHED upwind sum one
                                   by one, the reference's order :545, :624:
                                   in registers (plans at nx <= 66, device calls
                                   at nx <= 36 and nz <= 32: no extra memory, no
                                   extra kernel); the other cases -- larger nx,
                                   mpdata_plan_run_uw, device calls with nz 33 ..
                                   64 -- in a park
                                   array of the size of f's interior per tracer
                                   (with the plan, or kept per host thread and
                                   stream for device calls) that a
                                   finishing kernel adds.  MPDATA_EXACT_FLUX=sum
                                   in the environment does without either
                                   (=hbm: the park array everywhere; device calls
                                   on arrays of 4 GiB and more then do not park):
                                   flux is then the sum of the reference's terms in
                                   another order (sum of upwind terms + sum of
                                   limited terms, each in the reference's i
                                   order), equal to <= 1e-13 relative. */
#define MPDATA_VARIANT_FAST 1   /* FMA contraction allowed, Newton reciprocal in
                                   the limiter: differs from the above by
                                   rounding only (< 1e-12 abs on conditioned
                                   inputs, < 1e-14 relative L1 on the reference's
                                   own input law) */

/* ---- 1. Drop-in call: host arrays, synchronous, transfers included. -------
 * Replaces `call advect_scalar2D_openacc_N(f,u,w,rho,rhow,flux)` (reference
 * :53,:57) including its `!$acc update device/host` traffic (:107,:241).
 * Sizes and adz, which the reference routine takes by host association
 * (:7-30), are explicit arguments here. */
int mpdata_advect_scalar2d(int64_t ncrms, int nx, int nz, int ntracers,
                           double* f, const double* u, const double* w,
                           const double* rho, const double* rhow,
                           const double* adz, double* flux);
/* The call keeps what it needs besides the caller's arrays -- two streams and up to three sets of chunk
 * buffers (3/8 of the arrays' size at the default chunking) -- for the next call of the same HOST
 * THREAD (creating and destroying them costs 6.7 ms per call).  This releases the calling thread's
 * set; a thread that ends releases its own; MPDATA_HOST_CACHE=0 in the environment keeps nothing.
 * The same call releases the park arrays that EXACT calls on reference-layout DEVICE arrays keep per
 * host thread and stream (only where the limited fluxes do not fit registers: nx > 36, nz 33 .. 64), and
 * the wave-major plan that calls on reference-layout device arrays with 65 <= nz <= 238 run through
 * (the size of the call's arrays; kept per host thread for the next call of the same shape). */
int mpdata_release_host_buffers(void);

/* ---- 2. Device-resident call: device pointers, asynchronous on `stream`
 * (a hipStream_t passed as void*; NULL = the default stream).  This is the
 * reference's timed region (:110-238: kernels only, data already on the
 * device).  Arrays cover `ncrms` CRM instances with leading dimension
 * `ncrms`.  In-place on f.  nz <= 64: one kernel on the caller's arrays.
 * 65 <= nz <= 238: through a wave-major plan kept per host thread (import,
 * plan kernel, export, all on `stream`; the first call of a shape allocates;
 * MPDATA_DEVICE_CALL=direct: the k-marching kernel on the caller's arrays,
 * a third of the rate).  nz > 238: the k-marching kernel (fp64, nx <= 140), or
 * level windows (section 3e, when switched on).  fp32 with an odd ncrms: section 3f. */
int mpdata_advect_scalar2d_device(int64_t ncrms, int nx, int nz, int ntracers,
                                  double* f, const double* u, const double* w,
                                  const double* rho, const double* rhow,
                                  const double* adz, double* flux, void* stream);

/* ---- 3. Plan API: device state owned by the library (what the OpenACC
 * `enter data pcreate` / `update device` / `update host` directives do,
 * reference :105-107, :241, :662-663).  A plan lives on the device that is
 * current when it is created (every plan call switches to it and back), and
 * fixes the kernel variant at creation.
 *
 * Device layout.  The arrays a caller passes are ALWAYS in the reference
 * layout above.  Inside a plan with nz <= 238 (fp64; fp32 with an even ncrms, or any ncrms with section 3f on) the library keeps them in
 * its own "wave-major" order -- [tile of 64/LPS adjacent instances][column]
 * [instance][level], LPS = 8/16/32/64 >= nz (nz > 64: one instance per tile, worked on by several waves) -- so that
 * every wave streams contiguous memory; upload / download / import / export
 * convert on the device.  Other plans (nz > 238 unless section 3e is on; fp32 with an odd ncrms unless section 3f is on), MPDATA_PLAN_LAYOUT=
 * reference or mpdata_set_plan_layout(MPDATA_LAYOUT_REFERENCE) keep the
 * reference layout.  Results do not depend on the layout. */
#define MPDATA_LAYOUT_REFERENCE 0
#define MPDATA_LAYOUT_WAVEMAJOR 1
typedef struct mpdata_plan mpdata_plan;
int mpdata_plan_create(int64_t ncrms, int nx, int nz, int ntracers, mpdata_plan** plan);
int mpdata_plan_upload(mpdata_plan* plan, const double* f, const double* u, const double* w,
                       const double* rho, const double* rhow, const double* adz,
                       const double* flux);              /* host arrays; flux may be NULL */
int mpdata_plan_run(mpdata_plan* plan);            /* all tracers; async on the plan's stream */
int mpdata_plan_run_tracers(mpdata_plan* plan, int first_tracer, int ntracers); /* a sub-range */
/* One step on FRESH velocities: u, w are reference-layout DEVICE arrays of the plan's precision
 * (what a CRM whose state lives on the device produces every step; the reference's timed region
 * takes whatever u, w the device arrays hold, :107-110), f, rho, rhow, adz stay in the plan.
 * Entering the plan layout is part of the call and of its event time.  One fp64 tracer of a
 * wave-major plan: a kernel that reads u, w straight from the reference layout (128-byte row
 * segments through an LDS ring shared by the waves of a workgroup) while f streams in the
 * plan layout -- no conversion pass; other calls (tracer batches, fp32, odd ncrms, unaligned
 * bases ...) convert on the way.  On a multi-GPU plan u, w are full-width arrays on the root GPU:
 * they are scattered (section 3b), then every GPU runs.
 * POST-CONDITION (the same on every path): the plan holds NO velocities afterwards -- whether its
 * own u, w were left alone or overwritten depends on the path and is not promised.
 * mpdata_plan_run / _run_tracers return MPDATA_ESTATE until u AND w have been handed over again
 * (mpdata_plan_upload, or mpdata_plan_import_device with u and w); further mpdata_plan_run_uw
 * calls need nothing.  u and w count separately: a whole import of u alone after mpdata_plan_run_uw hands back u only, and
 * mpdata_plan_run stays at MPDATA_ESTATE until w has been imported whole as well (and the other way round). */
int mpdata_plan_run_uw(mpdata_plan* plan, int first_tracer, int ntracers, const void* u, const void* w);
int mpdata_plan_sync(mpdata_plan* plan);           /* the `!$acc wait` (:237) */
int mpdata_plan_download(mpdata_plan* plan, double* f, double* flux);  /* host arrays */
int mpdata_plan_last_kernel_ms(mpdata_plan* plan, double* ms); /* hipEvent time of the last run */
/* The event pair behind mpdata_plan_last_kernel_ms is recorded around EVERY run (two marker packets
 * between consecutive launches of a stream, about 1.5 % of a 0.4-ms kernel).  on = 0 switches it
 * off for callers that time a whole loop themselves; last_kernel_ms then returns MPDATA_ESTATE, from that call on and
 * until a run has been recorded with the pair switched on again (as it does before the plan's first run). */
int mpdata_plan_set_timing(mpdata_plan* plan, int on);
int mpdata_plan_destroy(mpdata_plan* plan);
/* Device-side exchange with a plan: reference-layout DEVICE arrays of the plan's precision on
 * the plan's device, asynchronous on the plan's stream.  Import: NULL pointers are skipped
 * (the plan keeps what it has); f and flux cover tracers [first_tracer, first_tracer+ntracers).
 * A caller whose state lives on the device imports once, runs many times, exports when it
 * needs the field back (several steps of one boundary condition: mpdata_plan_set_boundary, 3a). */
int mpdata_plan_import_device(mpdata_plan* plan, const void* f, const void* u, const void* w,
                              const void* rho, const void* rhow, const void* adz,
                              const void* flux, int first_tracer, int ntracers);
int mpdata_plan_export_device(mpdata_plan* plan, void* f, void* flux, int first_tracer, int ntracers);
/* Run on the caller's stream (hipStream_t as void*; NULL = default stream) from now on. */
int mpdata_plan_set_stream(mpdata_plan* plan, void* stream);
int mpdata_plan_layout(const mpdata_plan* plan);   /* MPDATA_LAYOUT_* */
int mpdata_plan_device(const mpdata_plan* plan);   /* HIP device ordinal */
int mpdata_set_plan_layout(int layout);            /* default for new plans; returns previous */

/* ---- 3a. Lateral boundary of a plan.  The routine reads f's halo columns -2..0 and nx+1..nx+3 as
 * INPUTS (the caller's boundary exchange fills them before every call) and leaves first-pass values in
 * -1, 0, nx+1, nx+2 (see the array contract above), so a second run of a GIVEN plan does not step any
 * boundary condition.  MPDATA_BOUNDARY_PERIODIC (the CRMs of the MMF are periodic in x): in front of
 * EVERY run (run, run_tracers, run_uw) and every read-back of f (download, export_device, the
 * multi-GPU gather) the halo columns of the tracers concerned become copies of the interior --
 * column i takes column 1 + ((i-1) mod nx), at every level, any nx >= 1 -- so K runs are K steps of
 * `wrap(f); advect(f)` and f comes back wrapped (EXACT: bit-identical to that loop, flux included).
 * Halo columns are not state in this mode: imported halos are ignored.  u and w are used as given
 * (periodic flow: wrap them with mpdata_periodic_halo_device); flux is unaffected.  The refresh is
 * one small kernel in the run's event pair (its tracers only, and only where a run or an import
 * since the last refresh left the halos stale).  set_boundary(GIVEN) on a periodic plan first wraps,
 * so the plan then holds what an export just before the switch would have returned.  Multi-GPU
 * plans forward the mode to every shard.  Default: GIVEN, today's behaviour exactly. */
#define MPDATA_BOUNDARY_GIVEN 0
#define MPDATA_BOUNDARY_PERIODIC 1
int mpdata_plan_set_boundary(mpdata_plan* plan, int mode); /* 0, or MPDATA_EINVAL (null plan, unknown mode) */
int mpdata_plan_boundary(const mpdata_plan* plan);        /* MPDATA_BOUNDARY_*; MPDATA_EINVAL for a null plan */

/* ---- 3c. Periodic halos of reference-layout DEVICE arrays, in place, asynchronous on `stream`
 * (NULL = default stream): f in columns -2..0, nx+1..nx+3 (ntracers tracers); u in columns -1, 0,
 * nx+1..nx+3 (every level); w in columns -1, 0, nx+1, nx+2 (all nz levels) -- column i := column
 * 1 + ((i-1) mod nx).  Any of f, u, w may be NULL, not all three.  Arguments are checked before any
 * device call (MPDATA_EINVAL). */
int mpdata_periodic_halo_device(int64_t ncrms, int nx, int nz, int ntracers, double* f, double* u, double* w,
                                void* stream);
int mpdata_periodic_halo_f32_device(int64_t ncrms, int nx, int nz, int ntracers, float* f, float* u, float* w,
                                    void* stream);

/* ---- 3b. One problem on several GPUs of the node.  No statement of the routine couples two
 * CRM instances (reference :505-637), so the ncrms axis is cut into `ngpus` contiguous blocks
 * (mpdata_shard_range), each GPU runs a plan of its own on its block and there is NO data-path
 * collective.  What replaces the reference's `!$acc update device / update host` (:107,
 * :241-242) depends on where the global arrays live:
 *   on the ROOT GPU (shard 0's device; mpdata_plan_import_device / _export_device on the
 *   multi-GPU plan, full-width reference-layout arrays): scatter = pack kernel (a block is a
 *   strided slab: `sl` is the fastest axis) + ncclSend / ncclRecv in ONE group -- RCCL over
 *   xGMI, one direct link per peer --, gather the reverse;
 *   on the HOST (mpdata_plan_upload / _download): every GPU copies its own slab ("direct": all
 *   PCIe links in parallel, nothing funnels through the root's one link).
 * One host thread drives all devices; the arrays of one transfer are queued back to back and
 * synchronised once.  The handle is an ordinary plan: upload, import_device, run, run_tracers,
 * sync, download, export_device, last_kernel_ms (slowest GPU) and destroy work on it; results
 * are bitwise those of a single-GPU plan.  MPDATA_MULTI_XFER = rccl | p2p (hipMemcpyPeerAsync)
 * | direct forces one transport for both origins (direct: host arrays only). */
int mpdata_plan_create_multi(int64_t ncrms, int nx, int nz, int ntracers, int ngpus, mpdata_plan** plan);
int mpdata_plan_create_multi_devices(int64_t ncrms, int nx, int nz, int ntracers, int ngpus,
                                     const int* devices, mpdata_plan** plan); /* explicit HIP ordinals */
void mpdata_shard_range(int64_t ncrms, int ngpus, int g, int64_t* sl0, int64_t* nloc); /* block of GPU g */
int mpdata_plan_ngpus(const mpdata_plan* plan);
int mpdata_plan_ranks_seen(const mpdata_plan* plan); /* ncclCommCount of the plan's communicator; 0: none */
int mpdata_plan_shard(const mpdata_plan* plan, int g, int* device, int64_t* sl0, int64_t* nloc);
/* the single-device plan of GPU g (owned by the multi-GPU plan: do not destroy): for callers whose
 * shard already lives on that device -- mpdata_plan_import_device / _export_device on it */
mpdata_plan* mpdata_plan_shard_plan(mpdata_plan* plan, int g);
/* wall seconds and bytes per peer link of the last upload (scatter) / download (gather);
 * transport (of the last transfer): 0 rccl, 1 p2p, 2 direct */
int mpdata_plan_transfer_stats(const mpdata_plan* plan, double* scatter_s, double* gather_s,
                               int64_t* scatter_bytes_per_peer, int64_t* gather_bytes_per_peer,
                               int* transport);

/* ---- 3d. Blocks of CRM instances of a resident plan.  No statement of the routine couples two instances (3b), so
 * instances [sl0, sl0+n) of a plan are a complete problem (n, nx, nz, ntracers) of their own; these calls move one in
 * or out at the cost of the block, not of the plan (the grid of the conversion kernel covers the tiles the block
 * touches; time per call on the MI355X: not measured yet, docs/EXPERIMENTS.md E).  The arrays are reference-layout arrays of the
 * plan's precision that cover ONLY the block: exactly the arrays of a problem of n instances, leading dimension n,
 * not ncrms.  Any 0 <= sl0, 1 <= n, sl0 + n <= ncrms: a block need not respect the plan's tiles, the instance pairs
 * of fp32 plans (the partner of a split pair keeps its value), or any alignment beyond that of a real.  Both plan
 * layouts, both precisions.  An fp32 plan with an odd ncrms on the packed kernels (section 3f) takes blocks like any other;
 * one that ends on the plan's last instance, sl0 + n == ncrms, also refreshes the plan's phantom half.
 *   export / download: exactly the slice [sl0, sl0+n) along the instance axis of what mpdata_plan_export_device /
 *     _download of the whole plan would return at that moment -- every element of f (halo columns included; a
 *     PERIODIC plan hands them out wrapped) and all nz levels of flux.
 *   import: replaces exactly those instances of the arrays given (NULL: skipped); every other instance and every
 *     other array stay bit-identical, and the plan then behaves as if the whole arrays with the slice replaced had
 *     been imported.  PERIODIC plans: an f block marks the halos of its tracers stale and imported halos are
 *     ignored, as with a whole import; GIVEN plans take the block's halos as given.
 * The device forms are asynchronous on the plan's stream; the host forms cover all tracers and are synchronous.
 * State: a plan cannot be FIRST filled block by block -- "filled" and "holds velocities" stay facts about the whole
 * plan: MPDATA_ESTATE until one mpdata_plan_upload / whole mpdata_plan_import_device has run, for a u or w block
 * while the plan holds no velocities (after mpdata_plan_run_uw), and for a host form of the other precision.  A u block
 * needs whole u to be held and a w block whole w, each on its own: while only w is held a u block returns MPDATA_ESTATE
 * and a w block is taken.
 * MPDATA_EINVAL (before any device call): null plan, n < 1, a range outside [0, ncrms), a bad tracer range, all
 * pointers NULL.  A multi-GPU handle returns MPDATA_EUNSUPPORTED: take the single-device plan of a shard
 * (mpdata_plan_shard_plan) and a shard-local sl0. */
int mpdata_plan_import_instances_device(mpdata_plan* plan, int64_t sl0, int64_t n,
                                        const void* f, const void* u, const void* w, const void* rho,
                                        const void* rhow, const void* adz, const void* flux,
                                        int first_tracer, int ntracers);
int mpdata_plan_export_instances_device(mpdata_plan* plan, int64_t sl0, int64_t n, void* f, void* flux,
                                        int first_tracer, int ntracers);
int mpdata_plan_download_instances(mpdata_plan* plan, int64_t sl0, int64_t n, double* f, double* flux);
int mpdata_plan_download_instances_f32(mpdata_plan* plan, int64_t sl0, int64_t n, float* f, float* flux);

/* ---- 3e. Tall columns: plans with nz > 238 as overlapping windows of at most 64 levels.  The routine's dependency
 * cone has radius 3 in k, so a window of levels computes the levels that lie 3 or more inside its artificial edges
 * exactly, from its own levels alone.  With the switch ON, mpdata_plan_create[_f32] with nz > 238 (fp64; fp32 with an
 * even ncrms) makes a WINDOWED plan: a wave-major plan of ncrms * W pseudo-instances of nz_w <= 64 levels (window index
 * fastest; the overlap levels are stored twice, about 64/57 of the memory), which the plan kernel of nz <= 64 runs.
 * mpdata_plan_layout() reports MPDATA_LAYOUT_WAVEMAJOR for it and every plan call keeps its contract: the arrays a
 * caller passes stay tall reference-layout arrays (split on the way in, the OWNED levels of every window merged on
 * the way out); between two runs one small kernel copies each window's non-owned levels of f from their owners (only
 * for tracers whose seams a run has left stale, inside the run's event pair, in front of the periodic wrap).  Results
 * are those of a tall plan (EXACT: bit-identical, flux included).  Also lifts the limits of the k-marching fall-back:
 * fp32, nx > 140 and k-planes of 2 GiB and more work.  The device and host calls (sections 1, 2, 6) on nz > 238 go
 * through such a plan kept per host thread while the switch is on.  nz <= 238, fp32 plans with an odd ncrms (unless
 * section 3f is on as well: the inner plan of ncrms * W pseudo-instances is then padded by its rule when that product is
 * odd) and MPDATA_PLAN_LAYOUT=reference / mpdata_set_plan_layout(MPDATA_LAYOUT_REFERENCE) are not affected.
 * Default OFF: today's behaviour exactly (MPDATA_TALL_COLUMNS=1 in the environment presets ON). */
int mpdata_set_tall_columns(int on);                 /* returns the previous setting */
int mpdata_plan_level_windows(const mpdata_plan* plan); /* W; 1 for every plan that is not windowed; multi-GPU: of shard 0 */
/* The geometry, pure arithmetic (no device): window h of the W = return value windows of a column of nz levels is a
 * problem of *nz_w levels whose real levels 1 .. nz_w-1 are the tall levels k0+1 .. k0+nz_w-1, and whose results are
 * used at the tall levels *own0 .. *own1 (1-based; the owned ranges tile 1 .. nz-1).  nz <= 64: W = 1, the whole
 * column.  Any pointer may be NULL.  MPDATA_EINVAL: nz < 2, or h outside [0, W). */
int mpdata_level_window(int nz, int h, int* k0, int* nz_w, int* own0, int* own1);

/* ---- 3f. fp32 with an odd ncrms on the packed kernels.  The fp32 kernels hold two adjacent instances per lane, so
 * without this switch an odd ncrms gets a reference-layout plan on the one-instance-per-lane kernel at nz <= 32 and
 * MPDATA_EUNSUPPORTED above.  No statement of the routine couples two instances (3b): a problem of ncrms + 1 instances
 * whose last instance repeats instance ncrms - 1 computes instances 0 .. ncrms-1 of the odd problem bit for bit.  With
 * the switch ON, mpdata_plan_create_f32 with an odd ncrms and 3 <= nz <= 238 makes a wave-major plan of (ncrms + 1) / 2
 * pairs -- the same kernels and forms as an even plan (LPS 8 .. 64, several waves per instance above 64 levels) -- whose
 * last pair has a PHANTOM upper half: always a copy of instance ncrms - 1 in every plan array (the padding pairs of the
 * last tile are copies of that pair), refreshed by every import, whole or block, that replaces that instance, and never
 * handed to the caller.  mpdata_plan_layout() reports MPDATA_LAYOUT_WAVEMAJOR and every plan call of sections 3, 3a, 3d
 * keeps its contract on arrays of leading dimension ncrms: the whole-plan conversions of such a plan move single reals on
 * the reference side (4-byte row accesses bounded by ncrms; no byte outside [array, array + ncrms * rows * 4) is loaded
 * or stored, at any 4-byte aligned base) and whole pairs on the plan side.  With section 3e on as well, nz > 238 works
 * for an odd ncrms.  mpdata_advect_scalar2d_f32_device / mpdata_advect_scalar2d_f32 with an odd ncrms: nz 33 .. 238 (and
 * above with 3e) through the calling thread's staged plan, as nz 65 .. 238 of an even ncrms; nz <= 32 stays on the direct
 * one-instance-per-lane kernel, which needs no second copy of the problem.  MPDATA_DEVICE_CALL=direct, MPDATA_PLAN_LAYOUT=
 * reference, mpdata_set_plan_layout(MPDATA_LAYOUT_REFERENCE) and a tile override keep their meaning and their errors.
 * fp64 and multi-GPU plans (fp64 only) are not affected.  Results: those of the odd problem (EXACT: bit-identical, flux
 * included).  Default OFF: today's behaviour exactly (MPDATA_F32_ODD_NCRMS=1 in the environment presets ON). */
int mpdata_set_f32_odd_ncrms(int on);                /* returns the previous setting */

/* ---- 3g. Horizontal statistics of a resident plan's tracers: per tracer t, instance sl and level k = 1 .. nzm, over
 * the INTERIOR columns i = 1 .. nx of f (what a host model takes back from its CRMs: the horizontal mean, the extrema):
 *   sum(sl,k,t)   s = +0.0; do i = 1, nx: s = s + f(sl,i,k,t) -- in the plan's precision and exactly this order, the way
 *                 the reference forms flux (:541-546); no multiplication, so EXACT and FAST plans give the same bits
 *   min, max      the smallest / largest of those nx values, the bits of the chosen element (the sign of a zero result
 *                 is unspecified when both +0 and -0 occur; NaN is outside the contract)
 * Halo columns are never read: a PERIODIC plan needs no wrap, and nothing of a plan's state changes -- the calls read f
 * and write the outputs, whether or not the plan holds velocities, outside the run's event pair (filled, have_u, have_w,
 * halo and seam marks, the timing pair and last_kernel_ms stay as they are).  A kernel of its own on every kind of plan:
 * not fused into the run, nothing kept between calls.  Wave-major plans are read in place (a wave walks the interior
 * columns of its tile's chunk as a linear stream, the running values in registers); windowed plans (3e) write every
 * window's OWNED levels to the tall level they stand for -- right after a run whatever the seams hold, so no refresh is
 * launched; the phantom half of an odd fp32 plan (3f) and the padding of the last tile reach no output.
 * Outputs: reference-layout arrays of the plan's precision, (n, nzm [, ntracers]), instance index fastest, leading
 * dimension n, tightly packed, tracer slowest; any of the three may be NULL and is skipped.  No byte outside n * nzm *
 * ntracers reals of an output is touched.
 * MPDATA_EINVAL (before any device call): null plan, n < 1, a range outside [0, ncrms), a bad tracer range, all three
 * outputs NULL; bad sizes (ncrms < 1, nx < 1, nz < 2, ntracers < 1) or a null f in the array forms.  MPDATA_ESTATE: a plan
 * never filled (no upload and no whole import), a host form of the other precision.  A multi-GPU handle returns
 * MPDATA_EUNSUPPORTED as in 3d: take mpdata_plan_shard_plan(plan, g) and a shard-local sl0.
 * Time on the MI355X (docs/EXPERIMENTS.md J, tools/level_stats_bench.py): at ncrms = 65536, nx = 32, nz = 28, cold, one tracer,
 * all three outputs: fp64 0.121 ms = 3.7 TB/s of the nx * nzm * ncrms * 8 bytes it has to read, 0.58 of the 0.208 ms that
 * mpdata_plan_export_device of f alone takes; fp32 0.070 ms (3.2 TB/s), 0.63 of its export's 0.112 ms; 25 tracers: 2.91 ms
 * fp64 (0.57), 1.65 ms fp32 (0.66); a block of 64 instances: 0.008 ms. */
/* instances [sl0, sl0+n) of a resident plan; whole plan: sl0 = 0, n = ncrms.  Device arrays on the plan's device,
 * asynchronous on the plan's stream. */
int mpdata_plan_level_stats_device(mpdata_plan* plan, int64_t sl0, int64_t n, void* sum, void* mn, void* mx,
                                   int first_tracer, int ntracers);
/* host arrays, all tracers, synchronous (staging buffer owned by the plan, allocated by the first call, freed by destroy) */
int mpdata_plan_level_stats(mpdata_plan* plan, int64_t sl0, int64_t n, double* sum, double* mn, double* mx);
int mpdata_plan_level_stats_f32(mpdata_plan* plan, int64_t sl0, int64_t n, float* sum, float* mn, float* mx);
/* the same reduction on a reference-layout DEVICE array f(ncrms,-2:nx+3,1,nzm[,ntracers]), asynchronous on `stream`
 * (one thread per instance, 64-bit offsets: arrays of 4 GiB and more) */
int mpdata_level_stats_device(int64_t ncrms, int nx, int nz, int ntracers, const double* f,
                              double* sum, double* mn, double* mx, void* stream);
int mpdata_level_stats_f32_device(int64_t ncrms, int nx, int nz, int ntracers, const float* f,
                                  float* sum, float* mn, float* mx, void* stream);

/* ---- 3h. Outflow Courant number of a plan's velocities (the question a time loop asks before every step: are these
 * velocities stable for this step, or does it have to be subcycled -- SAM's kurant).  The routine's first pass, the
 * upwind step (:528-560), updates a cell as f(i,k) - (uuu(i+1) - uuu(i) + (www(k+1) - www(k)) * iadz) * irho; the
 * coefficient of f(i,k) in it is 1 - c, and the pass keeps the sign of f exactly where c <= 1.  For instance sl, interior
 * column i = 1 .. nx and level k = 1 .. nzm:
 *   a = max(0, u(sl,i+1,k)) - min(0, u(sl,i,k))
 *   b = max(0, wk1) - min(0, w(sl,i,k))          wk1 = w(sl,i,k+1) for k < nzm, and +0 for k = nzm
 *   c = (a + b * iadz) * irho                    iadz = 1 / adz(sl,k), irho = 1 / rho(sl,k)
 * wk1 = +0 at k = nzm because the routine sets www(:,:,:,nz) = 0 (:511): the caller's w(:,:,:,nz) is never read.  Every
 * operation is one correctly rounded operation in the plan's precision, in exactly this association and without
 * contraction, the divides IEEE divides: EXACT and FAST plans give the same bits.  c is mathematically >= 0; a zero is
 * stored as +0.0 whatever signed zeros u, w hold (the sign is cleared before anything is stored).  NaN or infinite
 * inputs and rho or adz <= 0 are outside the contract.
 *   clev(sl,k)   the max of c over i = 1 .. nx; reference layout (n, nzm), leading dimension n, tightly packed
 *   cinst(sl)    the max of clev(sl,k) over k = 1 .. nzm; n reals
 * Either output may be NULL (skipped), not both.  A max does not depend on the order, so both are defined bit for bit.
 * Only the velocity columns 1 .. nx+1 of u and 1 .. nx of w are read, never the halos (a periodic caller's halo cells
 * repeat interior ones).  A kernel of its own on every kind of plan (wave-major: a wave walks the column slots of u and
 * w of its tile's chunk, u(i+1) carried over, w(k+1) through an address of its own; windowed plans (3e) write their
 * OWNED levels; the phantom half of an odd fp32 plan (3f) and the padding reach no output); cinst is zeroed on the
 * call's stream and formed by an unsigned atomic max on the bit pattern (c >= +0).  Nothing of a plan's state changes
 * (filled, have_u, have_w, halo and seam marks, the timing pair and last_kernel_ms stay), outside the run's event pair.
 * No byte outside n * nzm reals of clev and n reals of cinst is touched.
 * MPDATA_EINVAL (before any device call): null plan, n < 1, a range outside [0, ncrms), both outputs NULL; bad sizes
 * (ncrms < 1, nx < 1, nz < 2) or a null u, w, rho, adz in the array forms.  MPDATA_ESTATE: a plan never filled, a plan
 * that does not hold both u and w (after mpdata_plan_run_uw, until both have been imported again), a host form of the
 * other precision.  A multi-GPU handle returns MPDATA_EUNSUPPORTED as in 3d and 3g.
 * Time on the MI355X (docs/EXPERIMENTS.md K, tools/courant_bench.py): not measured yet. */
/* instances [sl0, sl0+n) of a resident plan, the velocities the plan holds; device arrays of the plan's precision on the
 * plan's device, asynchronous on the plan's stream */
int mpdata_plan_courant_device(mpdata_plan* plan, int64_t sl0, int64_t n, void* clev, void* cinst);
/* host arrays, synchronous (the plan's block staging buffer, as the 3g host forms) */
int mpdata_plan_courant(mpdata_plan* plan, int64_t sl0, int64_t n, double* clev, double* cinst);
int mpdata_plan_courant_f32(mpdata_plan* plan, int64_t sl0, int64_t n, float* clev, float* cinst);
/* the same reduction on reference-layout DEVICE arrays u(ncrms,-1:nx+3,1,nzm), w(ncrms,-1:nx+2,1,nz), rho(ncrms,nzm),
 * adz(ncrms,nzm) -- the fresh u, w a caller is about to hand to mpdata_plan_run_uw, with the rho, adz it imported --
 * asynchronous on `stream` (one thread per instance, 64-bit offsets: arrays of 4 GiB and more) */
int mpdata_courant_device(int64_t ncrms, int nx, int nz, const double* u, const double* w, const double* rho,
                          const double* adz, double* clev, double* cinst, void* stream);
int mpdata_courant_f32_device(int64_t ncrms, int nx, int nz, const float* u, const float* w, const float* rho,
                              const float* adz, float* clev, float* cinst, void* stream);

/* ---- 3i. Per-level increments of a resident plan's tracers, in place (the write side of 3g: what a host model hands
 * its CRMs every step -- SAM's large-scale forcing f(i,k) = f(i,k) + dt * tend(k), relaxation, surface sources, the
 * correction of the mean after a GCM step: horizontally uniform, one value per instance, level and tracer).  For tracer
 * t in [first_tracer, first_tracer + ntracers), instance sl in [sl0, sl0 + n), level k = 1 .. nzm and EVERY column
 * i = -2 .. nx+3 (halo columns included):
 *   MPDATA_LEVEL_ADD        f(sl,i,k,t) = f(sl,i,k,t) + d(sl,k,t)
 *   MPDATA_LEVEL_ADD_CLIP   f(sl,i,k,t) = max(0, f(sl,i,k,t) + d(sl,k,t))      (the routine's own last statement, :634)
 * Each result is one correctly rounded add in the plan's precision, then the max; nothing multiplies, so EXACT and FAST
 * plans give the same bits.  ADD keeps the IEEE sign of a zero sum; in ADD_CLIP the sign of a zero result is unspecified
 * (hardware max); NaN and infinities are outside the contract.
 * d: a reference-layout array of the plan's precision, (n, nzm [, ntracers]), instance index fastest, leading dimension
 * n, tightly packed, tracer slowest -- exactly an output of 3g, so the two calls close the loop: mean out, tendency in.
 * It is only read, and no byte outside its n * nzm * ntracers reals is.
 * Afterwards the plan behaves exactly as if all of f had been exported, changed as above and imported again.  GIVEN
 * plans: the halos get the increment like any column.  PERIODIC plans: the increment is uniform in i, so wrapped halos
 * stay wrapped copies and an export hands out the wrapped result (the kernel writes every column slot; the halo marks
 * stay as they are).  Windowed plans (3e): every level a window stores, owned or not, takes the increment of the tall
 * level it stands for, so all stored copies of a tall level stay consistent and a run right after gives the tall
 * problem's bits.  Odd fp32 plans (3f): the phantom half follows instance ncrms - 1.  An fp32 block that splits a pair
 * leaves the partner's bits alone (no + 0.0, no clip: a -0.0 or a negative value there stays).  Every instance and tracer
 * outside the ranges, and flux, u, w, rho, rhow, adz, stay bit-identical.  Nothing else of a plan's state changes
 * (filled, have_u, have_w, the boundary mode, halo and seam marks, the timing pair and last_kernel_ms stay), outside the
 * run's event pair.  A kernel of its own on every kind of plan (wave-major: a wave walks all nx + 6 column slots of its
 * tile's chunk as a linear read-modify-write stream, its increment in a register); the plan kernels are not touched.
 * MPDATA_EINVAL (before any device call): null plan, null d, n < 1, a range outside [0, ncrms), a bad tracer range, an
 * unknown mode; bad sizes (ncrms < 1, nx < 1, nz < 2, ntracers < 1) or a null f in the array forms.  MPDATA_ESTATE: a plan
 * never filled, a host form of the other precision.  A multi-GPU handle returns MPDATA_EUNSUPPORTED as in 3d and 3g: take
 * mpdata_plan_shard_plan(plan, g) and a shard-local sl0.  A failed call changes nothing.
 * Time on the MI355X (docs/EXPERIMENTS.md L, tools/level_add_bench.py): not measured yet; the yardstick is
 * mpdata_plan_export_device + mpdata_plan_import_device of f alone, expected traffic 2 (nx+6) nzm ncrms elem bytes. */
#define MPDATA_LEVEL_ADD 0
#define MPDATA_LEVEL_ADD_CLIP 1
/* instances [sl0, sl0+n) of a resident plan; whole plan: sl0 = 0, n = ncrms.  d: a device array on the plan's device;
 * asynchronous on the plan's stream. */
int mpdata_plan_level_add_device(mpdata_plan* plan, int64_t sl0, int64_t n, const void* d, int mode, int first_tracer,
                                 int ntracers);
/* host d, all tracers, synchronous (the plan's block staging buffer, as the 3g / 3h host forms) */
int mpdata_plan_level_add(mpdata_plan* plan, int64_t sl0, int64_t n, const double* d, int mode);
int mpdata_plan_level_add_f32(mpdata_plan* plan, int64_t sl0, int64_t n, const float* d, int mode);
/* the same on a reference-layout DEVICE array f(ncrms,-2:nx+3,1,nzm[,ntracers]) with d (ncrms, nzm [, ntracers]),
 * asynchronous on `stream` (one thread per instance, 64-bit offsets: arrays of 4 GiB and more) */
int mpdata_level_add_device(int64_t ncrms, int nx, int nz, int ntracers, double* f, const double* d, int mode, void* stream);
int mpdata_level_add_f32_device(int64_t ncrms, int nx, int nz, int ntracers, float* f, const float* d, int mode, void* stream);

/* ---- 3j. Scale a resident plan's velocities in place, one factor per instance (the write side of 3h: SAM's kurant turns
 * the Courant number into ncycle and advects ncycle times on u / ncycle, w / ncycle; a plan's u and w have no export, so
 * the factor is applied where they lie).  For every instance sl in [sl0, sl0 + n):
 *   u(sl, :, :) = u(sl, :, :) * su(sl - sl0)        every column -1 .. nx+3 and level the plan stores
 *   w(sl, :, :) = w(sl, :, :) * sw(sl - sl0)        every column -1 .. nx+2 and level the plan stores
 * Each element takes one correctly rounded multiply in the plan's precision; a single multiply leaves nothing to
 * contract, so EXACT and FAST plans get the same bits.  su, sw: arrays of n reals of the plan's precision, only read;
 * either may be NULL, which leaves that array as it is.  The factors are used as given: they are not validated, and a
 * zero, negative or non-finite factor does what IEEE says.  A factor of 1 leaves every bit, and the results of a run, as
 * they were.  Scaling by 1/m and later by m is NOT the identity unless m is a power of two (two roundings): a caller
 * that wants the unscaled velocities back imports them again.
 * Nothing is fused into the run and nothing is kept between calls.  No plan state changes (filled, have_u, have_w, halo
 * and seam marks, the boundary mode, the stream, the timing pair and last_kernel_ms stay), outside the run's event pair;
 * f, flux, rho, rhow, adz and every instance outside the range keep every bit.  Windowed plans (3e): every window of an
 * instance, and every level a window stores whether owned or not, takes that instance's factor, so all stored copies of a
 * tall level change alike.  Odd fp32 plans (3f): the phantom half follows instance ncrms - 1.  An fp32 block that splits
 * a pair stores the partner's half back exactly as loaded (no multiply by 1).  A kernel of its own on every kind of plan
 * (wave-major: a wave walks the column slots of its tile's chunk as a linear read-modify-write stream, eight columns in
 * flight, its factor in a register; one launch per array); the plan kernels are not touched.
 * Checked before any device call, in this order -- a failed call changes nothing:
 * MPDATA_EINVAL: null plan, n < 1, a range outside [0, ncrms); su and sw both NULL; in the array forms bad sizes
 * (ncrms < 1, nx < 1, nz < 2), no array at all, a factor without its array or an array without its factor.
 * MPDATA_EUNSUPPORTED: a multi-GPU handle, as in 3d - 3i: take mpdata_plan_shard_plan(plan, g) and a shard-local sl0.
 * MPDATA_ESTATE: a host form of the other precision; a plan never filled; a plan that does not hold the array being
 * scaled (after mpdata_plan_run_uw it holds neither; only the arrays asked for are tested).
 * Time on the MI355X (docs/EXPERIMENTS.md M, tools/scale_uw_bench.py): not measured yet; the yardstick is
 * mpdata_plan_import_device of u and w alone, expected traffic about 4 (nx+6) nzm ncrms elem bytes. */
/* instances [sl0, sl0+n) of a resident plan; whole plan: sl0 = 0, n = ncrms.  su, sw: device arrays on the plan's device;
 * asynchronous on the plan's stream. */
int mpdata_plan_scale_uw_device(mpdata_plan* plan, int64_t sl0, int64_t n, const void* su, const void* sw);
/* host su, sw, synchronous (the plan's block staging buffer, as the 3g - 3i host forms) */
int mpdata_plan_scale_uw(mpdata_plan* plan, int64_t sl0, int64_t n, const double* su, const double* sw);
int mpdata_plan_scale_uw_f32(mpdata_plan* plan, int64_t sl0, int64_t n, const float* su, const float* sw);
/* the same on reference-layout DEVICE arrays u(ncrms,-1:nx+3,1,nzm), w(ncrms,-1:nx+2,1,nz) with su, sw (ncrms) -- for
 * callers of mpdata_plan_run_uw.  Every column and every level the shapes hold is scaled, level nz of w included.  u or w
 * may be NULL together with its factor.  Asynchronous on `stream` (one thread per instance, 64-bit offsets). */
int mpdata_scale_uw_device(int64_t ncrms, int nx, int nz, double* u, double* w, const double* su, const double* sw, void* stream);
int mpdata_scale_uw_f32_device(int64_t ncrms, int nx, int nz, float* u, float* w, const float* su, const float* sw, void* stream);

/* ---- 3k. Mass-weighted column integrals of a resident plan's tracers (what a host model takes from its CRMs along the
 * column: SAM's precipitable water, its cloud and ice water paths, and, summed over x, the mass a conservation check looks
 * at).  3g - 3j reduce or broadcast along x; this call reduces along the levels.  For instance sl in [sl0, sl0 + n),
 * interior column i = 1 .. nx and tracer t in [first_tracer, first_tracer + ntracers), in the plan's precision:
 *   wgt(sl,k)    = rho(sl,k) * adz(sl,k)                                      one rounded multiply
 *   path(sl,i,t) : s = +0.0; do k = 1, nzm:  s = s + wgt(sl,k) * f(sl,i,k,t)   the product rounded, then the add; no fma
 *   mass(sl,t)   : s = +0.0; do i = 1, nx:   s = s + path(sl,i,t)
 * Every operation is rounded once, in exactly this order and association and without contraction, so EXACT and FAST
 * plans give the same bits.  Multiplying by dz or dividing by nx is the caller's scalar.  NaN and infinities are outside
 * the contract; the sign of a zero result is whatever this sequence gives.
 *   path   reference layout (n, nx [, ntracers]), instance index fastest, leading dimension n, tightly packed, tracer
 *          slowest; interior columns only.  Required.
 *   mass   (n [, ntracers]); NULL: skipped.  Formed from path by a second kernel on the same stream.
 * No byte outside n * nx * ntracers reals of path and n * ntracers reals of mass is touched.  Halo columns are never read:
 * a PERIODIC plan needs no wrap.  Of a windowed plan (3e) only the OWNED levels of every window are read, each with its
 * window's own weights, in rising order of the tall level -- right after a run whatever the seams hold, so no refresh is
 * launched.  The phantom half of an odd fp32 plan (3f), the padding of the last tile and the partner of a pair an fp32
 * block's ends split reach no output.  Nothing of a plan's state changes (filled, have_u, have_w, halo and seam marks,
 * the timing pair and last_kernel_ms stay), outside the run's event pair; the plan need not hold velocities.
 * A kernel of its own on every kind of plan, not fused into the run, nothing kept between calls.  Wave-major plans: the
 * levels of an instance are the lanes of the layout and the sum is sequential in k, so a lane owns one (instance, column)
 * pair; a workgroup copies the column slots of 16 adjacent 8-byte elements of the instance axis through LDS as the linear
 * streams the other block calls read, with the products rho * adz, and every lane then sums its column from LDS -- no
 * reduction across lanes, which would change the association.  The windows of a tall plan are staged one after the
 * other, the running sums stay in registers.
 * MPDATA_EINVAL (before any device call): null plan, n < 1, a range outside [0, ncrms), a bad tracer range, a null path;
 * bad sizes (ncrms < 1, nx < 1, nz < 2, ntracers < 1) or a null f, rho, adz in the array forms.  MPDATA_ESTATE: a plan
 * never filled (no upload and no whole import), a host form of the other precision.  A multi-GPU handle returns
 * MPDATA_EUNSUPPORTED as in 3d and 3g - 3j: take mpdata_plan_shard_plan(plan, g) and a shard-local sl0.
 * Time on the MI355X (docs/EXPERIMENTS.md O, tools/column_path_bench.py): not measured yet, and the GPU tests have not yet run there; the yardstick is
 * mpdata_plan_export_device of f alone on the same plan (the call reads the same bytes and writes 1 / nzm of them). */
/* instances [sl0, sl0+n) of a resident plan; whole plan: sl0 = 0, n = ncrms.  Device arrays of the plan's precision on
 * the plan's device, asynchronous on the plan's stream. */
int mpdata_plan_column_path_device(mpdata_plan* plan, int64_t sl0, int64_t n, void* path, void* mass, int first_tracer,
                                   int ntracers);
/* host arrays, all tracers, synchronous (the plan's block staging buffer, as the 3g - 3j host forms) */
int mpdata_plan_column_path(mpdata_plan* plan, int64_t sl0, int64_t n, double* path, double* mass);
int mpdata_plan_column_path_f32(mpdata_plan* plan, int64_t sl0, int64_t n, float* path, float* mass);
/* the same on reference-layout DEVICE arrays f(ncrms,-2:nx+3,1,nzm[,ntracers]), rho(ncrms,nzm), adz(ncrms,nzm),
 * asynchronous on `stream` (one thread per instance, 64-bit offsets: arrays of 4 GiB and more) */
int mpdata_column_path_device(int64_t ncrms, int nx, int nz, int ntracers, const double* f, const double* rho,
                              const double* adz, double* path, double* mass, void* stream);
int mpdata_column_path_f32_device(int64_t ncrms, int nx, int nz, int ntracers, const float* f, const float* rho,
                                  const float* adz, float* path, float* mass, void* stream);

/* ---- 3l. Eddy diffusion of a resident plan's tracers, in place (the operator a host model applies to every tracer right
 * after the advection: SAM's diffuse_scalar2D, the sibling of the routine -- the last per-step operator that forced f out
 * of a resident plan).  For instance sl in [sl0, sl0 + n), tracer t in [first_tracer, first_tracer + ntracers), nzm = nz - 1,
 * every f on the right-hand side the value BEFORE the call (Jacobi), every operation rounded once in the plan's precision
 * in exactly this association, nothing contracted, the divide IEEE:
 *   Fx(i,k) = -((cx(sl,k) * (tkh(sl,i,k) + tkh(sl,i+1,k))) * (f(i+1,k) - f(i,k)))        i = 0 .. nx,  k = 1 .. nzm
 *   Fz(i,k) = -((cz(sl,k) * (tkh(sl,i,k) + tkh(sl,i,k+1))) * (f(i,k+1) - f(i,k)))        i = 1 .. nx,  k = 1 .. nzm - 1
 *   Fz(i,0) = sb(sl,i)   (+0 if sb is NULL)          Fz(i,nzm) = st(sl,i)   (+0 if st is NULL)
 *   ir(k)   = 1 / (rho(sl,k) * adz(sl,k))
 *   f(i,k)  = f(i,k) - ((Fx(i,k) - Fx(i-1,k)) + (Fz(i,k) - Fz(i,k-1)) * ir(k))           i = 1 .. nx,  k = 1 .. nzm
 *   zflux(sl,k',t) : s = +0; do i = 1, nx: s = s + Fz(i,k'-1)                            k' = 1 .. nz   (NULL: skipped)
 * Negating a product is exact, so the sign convention costs no rounding; EXACT and FAST plans give the same bits.  NaN and
 * infinities are outside the contract.  All arrays are of the plan's precision, reference layout, instance index fastest,
 * leading dimension n (the block's first instance at index 0), tightly packed:
 *   tkh   (n, 0:nx+1, nzm)     the eddy diffusivity, shared by all tracers of the call, used as given (NOT wrapped)
 *   cx    (n, nzm)             the caller's folded coefficient, in SAM's terms 0.5 dtn grdf_x(k) / dx^2
 *   cz    (n, nzm)             0.5 dtn grdf_z(k) / dz^2 * rhow(k+1) / adzw(k+1); cz(:, nzm) is never read
 *   sb,st (n, nx)              the scaled surface and top fluxes; either may be NULL
 *   zflux (n, nz [, ntracers]) the horizontal sum of the vertical flux through every interface; may be NULL
 * rho and adz are those the plan holds.  Only the interior columns i = 1 .. nx change; the halo columns 0 and nx+1 are
 * inputs, exactly as they are for the routine.  GIVEN plans: they are what the plan holds.  PERIODIC plans: stale halos
 * of the tracer range are wrapped before the kernel, as a run does, and the marks of the range are cleared afterwards,
 * so the next run or read-back hands out wrapped halos of the diffused field.  flux, u, w, rho, rhow, adz, the boundary
 * mode, every tracer outside the range and every slot outside the block keep every bit: the padding of the last tile, a
 * neighbour in a tile, the partner of a pair an fp32 block splits (stored back exactly as loaded).  The one exception, as
 * in 3i / 3j: the phantom half of an odd fp32 plan (3f) follows instance ncrms - 1 whenever the block holds it.  The plan
 * need not hold velocities; the call is outside the run's event pair.
 * A kernel of its own on every kind of plan, not fused into the run.  Wave-major plans: tkh is brought into the plan
 * layout once per call (the conversion kernels of an import of f, into a buffer the plan owns, grown on demand and freed with it); a
 * workgroup owns whole tiles, loads every column batch, its look-ahead column and the vertical neighbours in the slice
 * next door before a barrier and stores only after it, so the in-place update is race-free by construction.
 * Reference-layout plans and the array forms write the new interior to a scratch array and copy it back by a second
 * kernel on the same stream.
 * Checked before any device call, in this order -- a failed call changes nothing:
 * MPDATA_EINVAL: null plan, n < 1, a range outside [0, ncrms), a bad tracer range; null tkh, cx or cz; in the array forms
 * bad sizes (ncrms < 1, nx < 1, nz < 2, ntracers < 1) or a null f, rho, adz.  MPDATA_EUNSUPPORTED: a multi-GPU handle, as in
 * 3d - 3k (take mpdata_plan_shard_plan(plan, g) and a shard-local sl0); a WINDOWED plan (3e, nz > 238): tkh would have to be
 * cut into level windows and the seams refreshed -- the named follow-up, not built yet.  MPDATA_ESTATE: a host form of the
 * other precision; a plan never filled.
 * Time on the MI355X (docs/EXPERIMENTS.md P, tools/diffuse_bench.py), 65536 x 32 x 28, one tracer, cold: 0.50 ms fp64,
 * 0.26 ms fp32 -- 1.16 x and 1.18 x mpdata_plan_export_device + mpdata_plan_import_device of f alone, the yardstick (the old
 * route without the caller's kernel).  Algorithmic traffic: f read and written once, tkh read once (2.8 TB/s); the
 * conversion pass of tkh reads and writes it once more (4.7 TB/s of all bytes moved) and is what a next version drops. */
/* instances [sl0, sl0+n) of a resident plan; whole plan: sl0 = 0, n = ncrms.  Device arrays of the plan's precision on
 * the plan's device, asynchronous on the plan's stream. */
int mpdata_plan_diffuse_device(mpdata_plan* plan, int64_t sl0, int64_t n, const void* tkh, const void* cx, const void* cz,
                               const void* sb, const void* st, void* zflux, int first_tracer, int ntracers);
/* host arrays, all tracers, synchronous (the plan's block staging buffer, as the 3g - 3k host forms) */
int mpdata_plan_diffuse(mpdata_plan* plan, int64_t sl0, int64_t n, const double* tkh, const double* cx, const double* cz,
                        const double* sb, const double* st, double* zflux);
int mpdata_plan_diffuse_f32(mpdata_plan* plan, int64_t sl0, int64_t n, const float* tkh, const float* cx, const float* cz,
                            const float* sb, const float* st, float* zflux);
/* the same on instances [sl0, sl0+n) of reference-layout DEVICE arrays f(ncrms,-2:nx+3,1,nzm[,ntracers]), rho(ncrms,nzm),
 * adz(ncrms,nzm) (leading dimension ncrms); tkh, cx, cz, sb, st, zflux as above (leading dimension n).  Enqueued on
 * `stream`; the call allocates its scratch array and returns when the work is done and the scratch is freed. */
int mpdata_diffuse_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, double* f, const double* rho,
                          const double* adz, const double* tkh, const double* cx, const double* cz, const double* sb,
                          const double* st, double* zflux, void* stream);
int mpdata_diffuse_f32_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, float* f, const float* rho,
                              const float* adz, const float* tkh, const float* cx, const float* cz, const float* sb,
                              const float* st, float* zflux, void* stream);

/* ---- 3m. Large-scale vertical advection of a resident plan's tracers, in place (the per-step operator a host model
 * applies to every tracer with the large-scale vertical velocity: SAM's subsidence, first-order upwind along k with one
 * velocity per level).  This section is the specification; the reference tree has no such routine.  For instance sl in
 * [sl0, sl0 + n), tracer t in [first_tracer, first_tracer + ntracers), nzm = nz - 1, level k = 1 .. nzm, kb = max(1, k-1),
 * kc = min(nzm, k+1) and EVERY column slot i = -2 .. nx+3:
 *   dec(i,k) = cb(sl,k) * (f(i,k) - f(i,kb))  +  cc(sl,k) * (f(i,kc) - f(i,k))
 *   f(i,k)   = f(i,k) - dec(i,k)
 *   dsum(sl,k,t) : s = +0;  do i = 1, nx:  s = s + dec(i,k)                              (NULL: skipped)
 * Every f on the right-hand side is the value BEFORE the call (Jacobi).  Every operation is rounded once in the plan's
 * precision, in exactly this association: two subtractions, two products, their sum, the final subtraction.  Nothing is
 * contracted, so EXACT and FAST plans give the same bits.  NaN and infinities are outside the contract.  A field that is
 * constant in k keeps every bit for any cb, cc, except that a -0.0 may come back as +0.0 (the differences are +0, the
 * decrement is -0 where both coefficients are negative, and -0 - (-0) = +0).  All arrays are of the plan's precision,
 * reference layout, instance index fastest, leading dimension n (the block's first instance at index 0), tightly packed:
 *   cb,cc (n, nzm)              shared by the tracers of the call, both required.  In SAM's terms the caller folds
 *                               dtn wsub(k) / (dz adzw(k)) into cb where wsub(k) >= 0, with cc = 0 there, and
 *                               dtn wsub(k) / (dz adzw(k+1)) into cc where wsub(k) < 0, with cb = 0; both zero at k = 1
 *                               and k = nzm.  The library does not look at signs.
 *   dsum  (n, nzm [, ntracers]) the decrement summed over the interior columns in rising i -- what a host model
 *                               accumulates as its large-scale advective tendency; may be NULL
 * Towards the rest of a plan:
 *   halo marks   the operator is the same in every column and couples none, so it acts on halo slots as on any other:
 *     the wrapped halos of a PERIODIC plan stay wrapped copies (same bits in, same operations), stale ones stay stale,
 *     and the marks are not touched -- no wrap is launched before or after.
 *   windowed plans (3e, nz > 238) are supported.  An owned level reads one level outside the owned range, so the call
 *     first refreshes the seams of the tracers of the range that a run has left stale, as a run does.  It then writes
 *     OWNED levels only, each with the coefficients of the tall level it stands for, and dsum is written by the owner:
 *     every tall level once.  A margin of 3 levels exceeds the radius of 1, so the merged result equals the operator on
 *     the tall column bit for bit.  The non-owned copies are stale afterwards: the seam marks of the range are cleared
 *     and the next run refreshes them.
 *   odd fp32 plans (3f)  the phantom half takes the result of instance ncrms - 1 whenever the block holds it (on a
 *     windowed plan the phantom of the inner plan is restored behind the call, as after a seam refresh).
 *   untouched    an fp32 block that splits a pair stores the partner back as loaded; padding slots, neighbours in a tile,
 *     instances and tracers outside the ranges, flux, u, w, rho, rhow, adz, the held-velocity flags, the boundary mode and
 *     the timing pair keep every bit.  The call is outside the run's event pair; the plan need not hold velocities.
 * A kernel of its own on every kind of plan, not fused into the run.  Wave-major plans: cb(k), cc(k) sit in a lane's
 * registers, f is read once and written once; f(k +- 1) come by a shuffle of the values just loaded, at a wave's first and
 * last lane by a load.  Up to 64 levels a tile's column chunk is one wave's; above, a workgroup owns whole tiles and loads
 * every column batch and its edge neighbours before a barrier and stores only after it, so the in-place update is
 * race-free by construction.  Reference-layout plans and the array forms write the new rows to a scratch array (the
 * plan's diffusion buffer of 3l; an allocation of the call's own in the array forms) and copy them back by a second
 * kernel on the same stream.
 * Checked before any device call, in this order -- a failed call changes nothing:
 * MPDATA_EINVAL: null plan, n < 1, a range outside [0, ncrms), a bad tracer range, null cb or cc; in the array forms bad
 * sizes (ncrms < 1, nx < 1, nz < 2, ntracers < 1), a null f, then null cb or cc.  MPDATA_EUNSUPPORTED: a multi-GPU handle,
 * as in 3d - 3l (take mpdata_plan_shard_plan(plan, g) and a shard-local sl0).  MPDATA_ESTATE: a host form of the other
 * precision; a plan never filled.
 * Time on the MI355X (docs/EXPERIMENTS.md S, tools/subside_bench.py), 65536 x 32 x 28, one tracer, cold: 0.237 ms fp64,
 * 0.121 ms fp32 (4.5 / 4.4 TB/s of f read once and written once) -- 0.54 x and 0.51 x mpdata_plan_export_device +
 * mpdata_plan_import_device of f alone (the old route without the caller's kernel) and 1.03 x mpdata_plan_level_add_device,
 * which moves the same bytes without the stencil; dsum adds 8 %. */
/* instances [sl0, sl0+n) of a resident plan; whole plan: sl0 = 0, n = ncrms.  Device arrays of the plan's precision on
 * the plan's device, asynchronous on the plan's stream. */
int mpdata_plan_subside_device(mpdata_plan* plan, int64_t sl0, int64_t n, const void* cb, const void* cc, void* dsum,
                               int first_tracer, int ntracers);
/* host arrays, all tracers, synchronous (the plan's block staging buffer, as the 3g - 3l host forms) */
int mpdata_plan_subside(mpdata_plan* plan, int64_t sl0, int64_t n, const double* cb, const double* cc, double* dsum);
int mpdata_plan_subside_f32(mpdata_plan* plan, int64_t sl0, int64_t n, const float* cb, const float* cc, float* dsum);
/* the same on reference-layout DEVICE arrays f(ncrms,-2:nx+3,1,nzm[,ntracers]), cb, cc (ncrms,nzm), dsum
 * (ncrms,nzm[,ntracers]) (leading dimension ncrms).  Enqueued on `stream`; the call allocates its scratch array and
 * returns when the work is done and the scratch is freed. */
int mpdata_subside_device(int64_t ncrms, int nx, int nz, int ntracers, double* f, const double* cb, const double* cc,
                          double* dsum, void* stream);
int mpdata_subside_f32_device(int64_t ncrms, int nx, int nz, int ntracers, float* f, const float* cb, const float* cc,
                              float* dsum, void* stream);

/* ---- 3n. Sedimentation of a resident plan's tracers, in place (the per-step operator a host model applies to its
 * precipitating water: SAM's precip_fall, falling along k with a fall speed that differs in every cell).  This section is
 * the specification; the reference tree has no such routine.  For instance sl in [sl0, sl0 + n), tracer t in
 * [first_tracer, first_tracer + ntracers), interior column i = 1 .. nx, level k = 1 .. nzm, nzm = nz - 1:
 *   Fz(i,k)   = wp(sl,i,k,t) * f(i,k)                      k = 1 .. nzm   (the flux through the LOWER face of cell k,
 *                                                                          positive downward)
 *   Fz(i,nz)  = +0                                                        (nothing enters through the top)
 *   ir(k)     = 1 / (rho(sl,k) * adz(sl,k))                               (as in 3l; rho, adz are the plan's)
 *   f(i,k)    = f(i,k) - (Fz(i,k) - Fz(i,k+1)) * ir(k)
 *   psfc(sl,i,t)  = Fz(i,1)                                               (NULL: skipped) what reaches the surface
 *   pflux(sl,k,t) : s = +0;  do i = 1, nx:  s = s + Fz(i,k)     k = 1 .. nzm   (NULL: skipped)
 * Every f on the right-hand side is the value BEFORE the call (Jacobi).  Every operation is rounded once in the plan's
 * precision, in exactly this association; nothing is contracted and the divide is IEEE, so EXACT and FAST plans give the
 * same bits.  The library does not look at the sign of wp: in SAM's terms the caller folds rhow(k) v_t dtn / dz into it.
 * wp = 0 keeps every bit of f, except that a -0.0 may come back as +0.0.  NaN and infinities are outside the contract.
 * All arrays are of the plan's precision, reference layout, instance index fastest, leading dimension n (the block's
 * first instance at index 0), tightly packed:
 *   wp    (n, nx, nzm [, ntracers])   one field per tracer of the call, interior columns only; required
 *   psfc  (n, nx [, ntracers])        may be NULL
 *   pflux (n, nzm [, ntracers])       may be NULL
 * Towards the rest of a plan:
 *   halo marks   only interior columns change; halo columns are neither read nor written.  GIVEN plans: halos keep every
 *     bit.  PERIODIC plans: no wrap is launched before the call, because nothing couples in x; the halo marks of the
 *     range are cleared afterwards, so the next run or read-back hands out wrapped halos of the new field.
 *   windowed plans (3e, nz > 238) are supported.  An owned level reads f(k+1), one level outside the owned range, so the
 *     call first refreshes the seams of the tracers of the range that a run has left stale, as a run does.  It then
 *     writes OWNED levels only, each with wp and ir of the tall level it stands for; psfc is written by the owner of tall
 *     level 1, pflux by each level's owner.  The seam marks of the range are cleared afterwards.  wp is addressed by tall
 *     level directly from the caller's array: nothing is cut into windows.
 *   odd fp32 plans (3f)  the phantom half follows instance ncrms - 1 whenever the block holds it (on a windowed plan the
 *     phantom of the inner plan is restored behind the call, as in 3m).
 *   untouched    an fp32 block that splits a pair stores the partner back as loaded; padding slots, neighbours in a tile,
 *     instances and tracers outside the ranges, flux, u, w, rho, rhow, adz, the held-velocity flags, the boundary mode and
 *     the timing pair keep every bit.  The call is outside the run's event pair; the plan need not hold velocities.
 * A kernel of its own on every kind of plan, not fused into the run.  Wave-major and windowed plans: wp is read WHERE IT
 * LIES -- no conversion pass, no byte of it written to device memory, the plan's diffusion buffer not used.  A workgroup
 * owns the whole tiles of a group of 16 adjacent 8-byte elements of the instance axis (16 instances fp64, 32 fp32: a row
 * of wp of the group is whole 128-byte lines in an aligned whole-plan call; fewer where the levels would not fit 40 KiB
 * of LDS) and, per batch of columns, copies the group's rows of wp into LDS re-laid as [column][unit][level]; f is read
 * once and written once, Fz(k+1) comes by a shuffle of the products just formed, at a wave's last lane from a load; psfc
 * is one level's products, formed by a small kernel in front while f is the old field.
 * Every load of f precedes a barrier and every store follows it, so the in-place update is race-free by construction.
 * Reference-layout plans and the array forms write the new interior to a scratch array (the plan's diffusion buffer of
 * 3l; an allocation of the call's own in the array forms) and copy it back by a second kernel on the same stream.
 * Checked before any device call, in this order -- a failed call changes nothing:
 * MPDATA_EINVAL: null plan, n < 1, a range outside [0, ncrms), a bad tracer range, a null wp; in the array forms bad sizes
 * (ncrms < 1, nx < 1, nz < 2, ntracers < 1), a block outside the arrays, a null f, rho or adz, then a null wp.
 * MPDATA_EUNSUPPORTED: a multi-GPU handle, as in 3d - 3m (take mpdata_plan_shard_plan(plan, g) and a shard-local sl0).
 * MPDATA_ESTATE: a host form of the other precision; a plan never filled.  psfc and pflux may both be NULL.
 * Time on the MI355X (docs/EXPERIMENTS.md U, tools/sediment_bench.py), 65536 x 32 x 28, one tracer, cold: 0.324 ms fp64,
 * 0.168 ms fp32 -- 4.2 / 4.0 TB/s of the algorithmic bytes (the interior of f read once and written once, wp read once:
 * 3 nx nzm ncrms reals, 1.359 GB fp64).  Against the parent's calls in the same run: 0.75 x / 0.72 x
 * mpdata_plan_export_device + mpdata_plan_import_device of f alone (the old route without the caller's kernel), 1.40 x /
 * 1.44 x mpdata_plan_level_add_device (no per-cell field), 0.63 x / 0.62 x mpdata_plan_diffuse_device (a per-cell field of
 * the same size through a conversion pass).  Said plainly: the rate is still BELOW the 4.7 / 4.4 TB/s at which diffuse moves
 * all its bytes, the conversion pass included (by 10 % and 9 %), so the call is not bound by its bytes yet -- the staging
 * through LDS with one barrier per batch and one per round is.  psfc and pflux together add 25 %, most of it the psfc
 * kernel, whose reads of one level of f use two of seven 64-byte sectors of a column chunk. */
/* instances [sl0, sl0+n) of a resident plan; whole plan: sl0 = 0, n = ncrms.  Device arrays of the plan's precision on
 * the plan's device, asynchronous on the plan's stream. */
int mpdata_plan_sediment_device(mpdata_plan* plan, int64_t sl0, int64_t n, const void* wp, void* psfc, void* pflux,
                                int first_tracer, int ntracers);
/* host arrays, all tracers, synchronous (the plan's block staging buffer, as the 3g - 3m host forms) */
int mpdata_plan_sediment(mpdata_plan* plan, int64_t sl0, int64_t n, const double* wp, double* psfc, double* pflux);
int mpdata_plan_sediment_f32(mpdata_plan* plan, int64_t sl0, int64_t n, const float* wp, float* psfc, float* pflux);
/* the same on instances [sl0, sl0+n) of reference-layout DEVICE arrays f(ncrms,-2:nx+3,1,nzm[,ntracers]), rho(ncrms,nzm),
 * adz(ncrms,nzm) (leading dimension ncrms); wp, psfc, pflux as above (leading dimension n).  Enqueued on `stream`; the
 * call allocates its scratch array and returns when the work is done and the scratch is freed. */
int mpdata_sediment_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, double* f, const double* rho,
                           const double* adz, const double* wp, double* psfc, double* pflux, void* stream);
int mpdata_sediment_f32_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, float* f, const float* rho,
                               const float* adz, const float* wp, float* psfc, float* pflux, void* stream);

/* ---- 3o. Implicit vertical solves of a resident plan's tracers, in place (the implicit half of a vertical operator of a
 * host model: backward-Euler vertical diffusion, implicit subsidence, implicit damping or nudging -- a tridiagonal solve
 * along k per column).  This section is the specification; the reference tree has no such routine.  For instance sl in
 * [sl0, sl0 + n), tracer t in [first_tracer, first_tracer + ntracers), interior column i = 1 .. nx, nzm = nz - 1, the call
 * replaces f(i,.) by the solution x of
 *   lo(sl,k) x(k-1) + di(sl,k) x(k) + up(sl,k) x(k+1) = f(i,k)          k = 1 .. nzm
 * computed exactly as follows, each statement one rounded operation in the plan's precision, nothing contracted, the
 * divide IEEE:
 *   per (sl,k), independent of column and tracer:
 *     p(1) = 1 / di(1);                                          g(1) = up(1) * p(1)
 *     k = 2 .. nzm:   m = lo(k) * g(k-1);  d = di(k) - m;  p(k) = 1 / d;  g(k) = up(k) * p(k)     (g(nzm) is not used)
 *   per (sl,i,t), every f the value BEFORE the call:
 *     y(1) = f(i,1) * p(1)
 *     k = 2 .. nzm:   m = lo(k) * y(k-1);  r = f(i,k) - m;  y(k) = r * p(k)
 *     x(nzm) = y(nzm)
 *     k = nzm-1 .. 1: m = g(k) * x(k+1);   x(k) = y(k) - m
 *     f(i,k) = x(k)
 * lo, di, up (n, nzm): of the plan's precision, reference layout, instance index fastest, leading dimension n (the block's
 * first instance at index 0), tightly packed, shared by all columns and all tracers of the call; lo(:,1) and up(:,nzm) are
 * never read.  All three are required.
 * NO PIVOTING: a matrix that needs none is the caller's duty -- diagonal dominance, as every implicit diffusion or upwind
 * matrix has.  A zero pivot, NaN and infinities are outside the contract.  EXACT and FAST plans give the same bits.
 * lo = up = 0, di = 1 keeps every bit of f, except that a -0.0 may come back as +0.0 (0 * y is -0.0 for a negative y, and
 * -0.0 - -0.0 = +0.0).  In the caller's terms: lo = -a(k), up = -c(k), di = 1 + a(k) + c(k) is backward-Euler vertical
 * diffusion with a horizontally uniform diffusivity (the caller folds dtn K / dz^2 and the density weights into a and c: INTEGRATION.md); it is
 * also the implicit counterpart of 3m's cb, cc.  The library does not look at signs.
 * Towards the rest of a plan:
 *   halo marks   only interior columns are read or written.  No wrap is launched before the call, because nothing couples
 *     in x.  GIVEN plans: halos keep every bit.  PERIODIC plans: the halo marks of the range are cleared afterwards, so the
 *     next run or read-back hands out wrapped halos of the new field.
 *   windowed plans (3e, nz > 238) are supported.  Only OWNED levels are read and written, each with the coefficients of
 *     the tall level it stands for; the coefficients are addressed by tall level in the caller's arrays: nothing is cut
 *     into windows.  Owned levels are right whatever the seams hold (as 3k argues), so no seam refresh is needed in
 *     front; the seam marks of the range are cleared afterwards.  The recurrence crosses the windows in both directions:
 *     a workgroup walks the windows of its instances upward with y(k-1) carried, then downward with x(k+1) carried.  The
 *     merged result is the tall solve bit for bit.  This costs a second read and write of f on tall plans; a plain plan
 *     reads f once and writes it once.
 *   odd fp32 plans (3f)  the phantom half follows instance ncrms - 1 whenever the block holds it (on a windowed plan the
 *     phantom of the inner plan is restored behind the call, as in 3m / 3n).
 *   untouched    an fp32 block that splits a pair stores the partner back as loaded; padding slots, neighbours in a group,
 *     instances and tracers outside the ranges, flux, u, w, rho, rhow, adz, the held-velocity flags, the boundary mode and
 *     the timing pair keep every bit.  The call is outside the run's event pair; the plan need not hold velocities.
 * Kernels of their own on every kind of plan, not fused into the run.  A small kernel in front forms p and g once per call
 * (one thread per instance, sequential in k) into the plan's diffusion buffer of 3l (2 n nzm reals; an allocation of the
 * call's own in the array forms), so the divides stay out of the hot kernel and every column takes the same bits.
 * Wave-major and windowed plans: the lanes of the plan layout run along k, the recurrence too, so a workgroup stages the
 * column slots of 16 adjacent 8-byte elements of the instance axis (fewer where the levels would not fit 40 KiB of LDS)
 * and a batch of columns through LDS as 3k does, together with lo, p, g of those instances; a lane per (instance element,
 * column) sweeps up and down in LDS in place, and the waves store LDS back to f as the same linear streams.  Every global
 * load of a stage precedes a barrier and every global store follows the sweeps' barrier; workgroups own disjoint elements:
 * the in-place update is race-free by construction.  Reference-layout plans and the array forms: one thread per instance
 * and (column, tracer) row owns its column and sweeps it in place.
 * Checked before any device call, in this order -- a failed call changes nothing:
 * MPDATA_EINVAL: null plan, n < 1, a range outside [0, ncrms), a bad tracer range, a null lo, di or up; in the array forms
 * bad sizes (ncrms < 1, nx < 1, nz < 2, ntracers < 1), a block outside the arrays, a null f, then a null lo, di or up.
 * MPDATA_EUNSUPPORTED: a multi-GPU handle, as in 3d - 3n (take mpdata_plan_shard_plan(plan, g) and a shard-local sl0).
 * MPDATA_ESTATE: a host form of the other precision; a plan never filled.
 * Time on the MI355X (docs/EXPERIMENTS.md V, tools/vsolve_bench.py), 65536 x 32 x 28, one tracer, cold: 0.263 ms fp64,
 * 0.166 ms fp32 (the factor kernel included) -- 3.4 / 2.7 TB/s of the algorithmic bytes (the interior of f read once and
 * written once: 2 nx nzm ncrms reals, 0.906 GB fp64).  Against the parent's calls in the same run: 0.62 x / 0.74 x
 * mpdata_plan_export_device + mpdata_plan_import_device of f alone (the old route without the caller's kernel), 1.99 x /
 * 2.20 x mpdata_plan_column_path_device (the same staging, read only: the call costs two of them), 1.15 x / 1.44 x
 * mpdata_plan_level_add_device (the same bytes and six halo columns more, no staging).  A block of 64 instances: 0.018 ms.
 * Said plainly: the call is bound by the staging through LDS and its two barriers, not by its bytes -- only half of a
 * workgroup's lanes sweep (16 instances x 8 columns), and level_add moves 1.4 x the rate.  Tall plans are worse than the
 * plan: at 4096 x 32 x 300 (6 windows of 56 levels) 1.00 ms fp64, 0.70 ms fp32, 0.63 / 0.45 TB/s, 2.8 x / 2.3 x the export +
 * import of f -- 5.5 x the plain time per byte where two passes explain 2 x: a batch is 2 columns there, so 32 of 256 lanes
 * sweep, and lo, p, g are staged again for every window and pass.  On a tall plan the call still saves the caller's kernel
 * and the host-side bookkeeping, not time. */
/* instances [sl0, sl0+n) of a resident plan; whole plan: sl0 = 0, n = ncrms.  Device arrays of the plan's precision on
 * the plan's device, asynchronous on the plan's stream. */
int mpdata_plan_vsolve_device(mpdata_plan* plan, int64_t sl0, int64_t n, const void* lo, const void* di, const void* up,
                              int first_tracer, int ntracers);
/* host arrays, all tracers, synchronous (the plan's block staging buffer, as the 3g - 3n host forms) */
int mpdata_plan_vsolve(mpdata_plan* plan, int64_t sl0, int64_t n, const double* lo, const double* di, const double* up);
int mpdata_plan_vsolve_f32(mpdata_plan* plan, int64_t sl0, int64_t n, const float* lo, const float* di, const float* up);
/* the same on instances [sl0, sl0+n) of a reference-layout DEVICE array f(ncrms,-2:nx+3,1,nzm[,ntracers]) (leading
 * dimension ncrms); lo, di, up as above (leading dimension n).  Enqueued on `stream`; the call allocates its scratch array
 * and returns when the work is done and the scratch is freed. */
int mpdata_vsolve_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, double* f, const double* lo,
                         const double* di, const double* up, void* stream);
int mpdata_vsolve_f32_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, float* f, const float* lo,
                             const float* di, const float* up, void* stream);

/* ---- 3p. Per-cell sources of a resident plan's tracers, in place (the most general write path of a host model: an
 * increment that differs in every cell -- radiative heating t(i,k) = t(i,k) + qrad(i,k) * dtn, the tendency of a
 * microphysics or chemistry scheme the library does not own, a source confined to some columns, a perturbation; 3i
 * applies only increments that are uniform in x).  This section is the specification; the reference tree has no such
 * routine.  For instance sl in [sl0, sl0 + n), tracer t in [first_tracer, first_tracer + ntracers), interior column
 * i = 1 .. nx, level k = 1 .. nzm, nzm = nz - 1, with b = sl - sl0:
 *   p        = c * s(b,i,k,t)
 *   g        = f(sl,i,k,t) + p
 *   MPDATA_CELL_ADD_CLIP only:  g = max(0, g)
 *   dsum(b,k,t) :  a = +0;  do i = 1, nx:  a = a + (g - f_old(sl,i,k,t))             (NULL: skipped)
 *   f(sl,i,k,t) = g
 * Every operation is rounded once in the plan's precision, in exactly this association; nothing is contracted, so EXACT
 * and FAST plans give the same bits.  The factor c (a time step, a unit conversion) is passed by value, as a double to
 * the device form, which serves both precisions; it is rounded ONCE to the plan's precision before use (c = 0.1 on an
 * fp32 plan multiplies by (float)0.1).  MPDATA_CELL_ADD keeps the IEEE signs of zero (c = 0 or s = 0 keeps every bit of
 * f, except that -0 + +0 = +0); under MPDATA_CELL_ADD_CLIP the sign of a zero f is unspecified, as in 3i, but dsum is
 * still bit-defined: a running sum that starts at +0 never becomes -0.  NaN and infinities are outside the contract.
 * dsum is the increment actually APPLIED, summed over the interior columns in rising order; under _CLIP it differs from
 * c * s wherever the clip acted.  It is what a budget needs.
 * All arrays are of the plan's precision, reference layout, instance index fastest, leading dimension n (the block's
 * first instance at index 0), tightly packed, tracer slowest:
 *   s    (n, nx, nzm [, ntracers])   one field per tracer of the call, interior columns only; required, only read
 *   dsum (n, nzm [, ntracers])       may be NULL
 * No byte outside these arrays is read or written.  Afterwards the plan behaves exactly as if the interior of f had been
 * exported, changed as above and imported again.
 * Towards the rest of a plan:
 *   halo marks   only interior columns change; halo columns are neither read nor written.  GIVEN plans: halos keep every
 *     bit.  PERIODIC plans: no wrap is launched, because nothing couples in x; the halo marks of the range are cleared
 *     afterwards, so the next run or read-back hands out wrapped halos of the new field.
 *   windowed plans (3e, nz > 238) are supported.  The operator is pointwise, so no seam refresh is needed in front: an
 *     owned level is right whatever the seams hold (as 3k argues).  The scheme chosen: the call writes OWNED levels only,
 *     each with s of the tall level it stands for, and clears the seam marks of the range afterwards; the next run
 *     refreshes the other copies, whether the seams were fresh or stale at the call.  dsum of a level is written by that
 *     level's owner.  s is addressed by tall level directly from the caller's array: nothing is cut into windows.
 *   odd fp32 plans (3f)  the phantom half follows instance ncrms - 1 whenever the block holds it (on a windowed plan the
 *     phantom of the inner plan is restored behind the call, as in 3m / 3n).
 *   untouched    an fp32 block that splits a pair stores the partner back as loaded -- no + 0.0 and no clip reach it: a
 *     -0.0 or a negative value there stays; padding slots, neighbours in a tile, instances and tracers outside the
 *     ranges, flux, u, w, rho, rhow, adz, the held-velocity flags, the boundary mode and the timing pair keep every bit.
 *     The call is outside the run's event pair; the plan need not hold velocities.
 * A kernel of its own on every kind of plan, not fused into the run.  Wave-major and windowed plans: s is read WHERE IT
 * LIES, as 3n reads wp -- no conversion pass, no scratch buffer; f is read once and written once, s read once.  A
 * workgroup owns the whole tiles of a group of 16 adjacent 8-byte elements of the instance axis (fewer where the levels
 * would not fit 40 KiB of LDS) and, per batch of columns, copies the group's rows of s into one of TWO LDS buffers re-laid
 * as [column][unit][level].  A lane reads and writes its own element of f only, so f needs no ordering; the one barrier
 * of a batch orders the staging.  The kernel without dsum carries neither the sums nor their LDS.
 * Reference-layout plans and the array forms: one thread per instance and (level, tracer) row, in place, no scratch array.
 * Checked before any device call, in this order -- a failed call changes nothing:
 * MPDATA_EINVAL: null plan, n < 1, a range outside [0, ncrms), a bad tracer range, a null s, an unknown mode; in the array
 * forms bad sizes (ncrms < 1, nx < 1, nz < 2, ntracers < 1), a block outside the arrays, a null f, then a null s, then the mode.
 * MPDATA_EUNSUPPORTED: a multi-GPU handle, as in 3d - 3o (take mpdata_plan_shard_plan(plan, g) and a shard-local sl0).
 * MPDATA_ESTATE: a host form of the other precision; a plan never filled.
 * Time on the MI355X (docs/EXPERIMENTS.md W, tools/cell_add_bench.py, profiles/cell_add_bench.json), 65536 x 32 x 28, one
 * tracer, cold: 0.319 ms fp64, 0.163 ms fp32 -- 4.3 / 4.2 TB/s of the algorithmic bytes (the interior of f read once and
 * written once, s read once: 3 nx nzm ncrms reals, 1.359 GB fp64); the clip costs nothing, dsum 2 % fp64 and 15 % fp32.
 * Against existing calls in the same run: 0.75 x / 0.70 x mpdata_plan_export_device + mpdata_plan_import_device of f alone
 * (the old route without the caller's kernel), 1.40 x / 1.41 x mpdata_plan_level_add_device (no per-cell field), 1.01 x /
 * 1.00 x mpdata_plan_sediment_device (the same bytes, a stencil, a second barrier per round and an edge load more).
 * Said plainly: the call is NOT faster than sedimentation although it does less, so the barriers and the edge load were
 * not what bounds 3n; what did move the time is loading the next batch's s into registers while a batch computes
 * (0.396 -> 0.319 ms fp64).  Tall plans, 4096 x 32 x 300 (6 windows): 0.362 ms fp64, 0.251 ms fp32, 0.98 x / 0.82 x the
 * export + import of f and 0.82 x / 0.86 x sedimentation -- on a tall fp64 plan the call saves the caller's kernel and the
 * bookkeeping, hardly time. */
#define MPDATA_CELL_ADD 0
#define MPDATA_CELL_ADD_CLIP 1
/* instances [sl0, sl0+n) of a resident plan; whole plan: sl0 = 0, n = ncrms.  Device arrays of the plan's precision on
 * the plan's device, asynchronous on the plan's stream. */
int mpdata_plan_cell_add_device(mpdata_plan* plan, int64_t sl0, int64_t n, const void* s, double c, int mode, void* dsum,
                                int first_tracer, int ntracers);
/* host arrays, all tracers, synchronous (the plan's block staging buffer, as the 3g - 3o host forms) */
int mpdata_plan_cell_add(mpdata_plan* plan, int64_t sl0, int64_t n, const double* s, double c, int mode, double* dsum);
int mpdata_plan_cell_add_f32(mpdata_plan* plan, int64_t sl0, int64_t n, const float* s, float c, int mode, float* dsum);
/* the same on instances [sl0, sl0+n) of a reference-layout DEVICE array f(ncrms,-2:nx+3,1,nzm[,ntracers]) (leading
 * dimension ncrms); s, dsum as above (leading dimension n).  Asynchronous on `stream`; 64-bit offsets. */
int mpdata_cell_add_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, double* f, const double* s,
                           double c, int mode, double* dsum, void* stream);
int mpdata_cell_add_f32_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, float* f, const float* s,
                               float c, int mode, float* dsum, void* stream);

/* ---- 3q. A fused column step of a resident plan's tracers, in place (what a host model does to every column after the
 * advection step: tendencies and forcing, large-scale vertical advection, precipitation fall, the implicit vertical
 * operator -- 3p, 3m, 3n and 3o as ONE call with one read of f and one write, no intermediate field in device memory).
 * This section is the specification; the reference tree has no such routine.  For instance sl in [sl0, sl0 + n), tracer t
 * in [first_tracer, first_tracer + ntracers), INTERIOR column i = 1 .. nx, level k = 1 .. nzm, nzm = nz - 1, b = sl - sl0,
 * the call applies up to four stages in this FIXED ORDER.  Each stage reads the field the stage before left; inside a
 * stage every f on the right is the value BEFORE that stage (Jacobi), exactly as in the single calls:
 *   1. source    present when s != NULL            (3p)   p = c * s(b,i,k,t);  g = f(i,k) + p;  MPDATA_CELL_ADD_CLIP only:
 *                                                         g = max(0, g);  f(i,k) = g
 *   2. subside   present when cb, cc != NULL       (3m)   kb = max(1,k-1), kc = min(nzm,k+1):
 *                                                         f(i,k) = f(i,k) - (cb(b,k) * (f(i,k) - f(i,kb)) + cc(b,k) * (f(i,kc) - f(i,k)))
 *   3. sediment  present when wp != NULL           (3n)   Fz(k) = wp(b,i,k,t) * f(i,k);  Fz(nz) = +0;  ir(k) = 1 / (rho(sl,k) * adz(sl,k));
 *                                                         f(i,k) = f(i,k) - (Fz(k) - Fz(k+1)) * ir(k)
 *                                                         psfc(b,i,t) = Fz(1), of the field that ENTERS this stage (NULL: skipped)
 *   4. vsolve    present when lo, di, up != NULL   (3o)   the factors p, g and the sweeps y, x exactly as 3o states them
 * The order is SAM's: tendencies and forcing, then precipitation fall, then the implicit vertical operator.  A caller that
 * needs another order makes two calls.  Every operation is rounded once in the plan's precision, in the association the
 * single sections state, nothing contracted, the divides IEEE: EXACT and FAST plans give the same bits.  c is a double by
 * value, rounded ONCE to the plan's precision; mode is MPDATA_CELL_ADD or MPDATA_CELL_ADD_CLIP and is ignored without s.
 * On the interior columns the result is BIT FOR BIT what the sequence of the present single calls gives (mpdata_plan_
 * cell_add_device, mpdata_plan_subside_device, mpdata_plan_sediment_device, mpdata_plan_vsolve_device), the absent stages
 * left out.  The call deliberately differs from that sequence in two places:
 *   halo slots       3m alone also updates the six halo slots.  The fused call neither reads nor writes halo columns at
 *     all.  GIVEN plans: halos keep every bit.  PERIODIC plans: no wrap is launched in front, and the halo marks of the
 *     tracer range are cleared afterwards -- what the next run or read-back sees is identical to the sequence.
 *   horizontal sums  3p's and 3m's dsum and 3n's pflux are NOT offered.  They are sums over i in rising order, and in this
 *     staging the columns of a level lie on different lanes and in different workgroups.  A caller takes them from the
 *     single calls on a statistics step; f comes out the same.
 * All arrays are of the plan's precision, reference layout, instance index fastest, leading dimension n (the block's first
 * instance at index 0), tightly packed, tracer slowest:
 *   s, wp                (n, nx, nzm [, ntracers])   one field per tracer of the call, only read
 *   psfc                 (n, nx [, ntracers])        may be NULL; only with wp
 *   cb, cc, lo, di, up   (n, nzm)                    shared by the columns and the tracers; lo(:,1), up(:,nzm) never read
 * No byte outside these arrays is read or written.
 * Towards the rest of a plan, as 3o states it: the phantom half of an odd fp32 plan (3f) follows instance ncrms - 1
 * whenever the block holds it; the partner of a split fp32 pair is stored back as loaded -- no + 0.0 and no clip reach it;
 * padding slots, neighbours in a group, instances and tracers outside the ranges, flux, u, w, rho, rhow, adz, the
 * held-velocity flags, the boundary mode and the timing pair keep every bit.  The call is outside the run's event pair;
 * the plan need not hold velocities.
 * Kernels of their own (mpdata_column_step.hip), specialised on the set of present stages: an absent stage costs nothing.
 * Wave-major plans: the geometry and the copy stage of 3o -- a workgroup stages the column slots of 16 adjacent 8-byte
 * elements of the instance axis (fewer where the levels would not fit 40 KiB of LDS) and a batch of columns in LDS as
 * [column][unit][level]; a lane per (unit, column) sweeps its column in LDS in place: stages 1 - 3 and the forward sweep
 * of stage 4 share ONE upward pass with the old neighbours carried in registers, the backward sweep is a second pass; then
 * the waves store LDS back.  s, wp and the coefficient rows are read by the sweeping lanes straight from the caller's
 * arrays, the unit fastest (a row of 16 units is one 128-byte line); only 1 / (rho * adz) is a row of LDS.  No conversion
 * pass, no scratch in device memory but the 2 n nzm factors of stage 4 in the plan's diffusion buffer, as 3o.  Race
 * freedom: DESIGN.md 4.20.  Reference-layout plans and the array forms: one thread per instance and (column, tracer) row
 * owns its column and sweeps it in place in device memory; no scratch array.
 * Checked before any device call, in this order -- a failed call changes nothing:
 * MPDATA_EINVAL: null plan, n < 1, a range outside [0, ncrms), a bad tracer range (as 3p); no stage present; exactly one of
 * cb, cc; one or two of lo, di, up; psfc without wp; an unknown mode while s is given; in the array forms bad sizes, a block
 * outside the arrays, a null f, then the same, then a null rho or adz with wp.
 * MPDATA_EUNSUPPORTED: a multi-GPU handle, as in 3d - 3p (take mpdata_plan_shard_plan(plan, g) and a shard-local sl0); a
 * WINDOWED plan (3e: nz > 238 with tall columns on) -- the named follow-up: stages 2 and 3 need fresh seams of the field
 * stage 1 leaves, stage 4 crosses the windows twice, and tall plans are where 3o already loses to the round trip.  Use the
 * single calls there.
 * MPDATA_ESTATE: a host form of the other precision; a plan never filled.
 * Time on the MI355X (docs/EXPERIMENTS.md X, tools/column_step_bench.py, profiles/column_step_bench.json), 65536 x 32 x 28,
 * one tracer, cold, all four stages: 0.593 ms fp64, 0.417 ms fp32 -- 3.1 / 2.2 TB/s of the algorithmic bytes (f read and
 * written once, s and wp read once: 4 nx nzm ncrms reals, 1.81 GB fp64) -- against 1.147 / 0.622 ms for the four single
 * calls in the same run: 0.52 x / 0.67 x their sum (1.37 x / 1.77 x the export + import of f alone).  psfc costs nothing.
 * The single-stage forms against their siblings: source 0.91 x / 0.96 x mpdata_plan_cell_add_device, subside 1.17 x /
 * 1.47 x mpdata_plan_subside_device, sediment 1.04 x / 1.25 x mpdata_plan_sediment_device, vsolve 1.37 x / 1.31 x
 * mpdata_plan_vsolve_device.  Said plainly: the fused call halves the fp64 time of the chain but reaches 0.59 ms where
 * the bytes alone would allow 0.43 ms at 3n's rate, and a caller with ONE stage other than the source is better served by
 * the single call: 176 of 256 lanes sweep (16 units x 11 columns; 3o has 128), but every sweeping lane fetches its
 * coefficient rows and its s and wp level by level from L2 three levels ahead of a dependent chain, where 3m streams f
 * without LDS and 3o reads its rows from LDS. */
/* instances [sl0, sl0+n) of a resident plan; whole plan: sl0 = 0, n = ncrms.  Device arrays of the plan's precision on
 * the plan's device, asynchronous on the plan's stream. */
int mpdata_plan_column_step_device(mpdata_plan* plan, int64_t sl0, int64_t n, const void* s, double c, int mode,
                                   const void* cb, const void* cc, const void* wp, void* psfc, const void* lo, const void* di,
                                   const void* up, int first_tracer, int ntracers);
/* host arrays, all tracers, synchronous (the plan's block staging buffer, as the 3g - 3p host forms) */
int mpdata_plan_column_step(mpdata_plan* plan, int64_t sl0, int64_t n, const double* s, double c, int mode, const double* cb,
                            const double* cc, const double* wp, double* psfc, const double* lo, const double* di,
                            const double* up);
int mpdata_plan_column_step_f32(mpdata_plan* plan, int64_t sl0, int64_t n, const float* s, float c, int mode, const float* cb,
                                const float* cc, const float* wp, float* psfc, const float* lo, const float* di,
                                const float* up);
/* the same on instances [sl0, sl0+n) of a reference-layout DEVICE array f(ncrms,-2:nx+3,1,nzm[,ntracers]) (leading
 * dimension ncrms) with rho, adz (ncrms, nzm), required only with wp; the other arrays as above (leading dimension n).
 * Enqueued on `stream`, 64-bit offsets; asynchronous without stage 4 -- with it the call allocates the factors' scratch
 * array and returns when the work is done and the scratch is freed. */
int mpdata_column_step_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, double* f, const double* rho,
                              const double* adz, const double* s, double c, int mode, const double* cb, const double* cc,
                              const double* wp, double* psfc, const double* lo, const double* di, const double* up,
                              void* stream);
int mpdata_column_step_f32_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, float* f, const float* rho,
                                  const float* adz, const float* s, float c, int mode, const float* cb, const float* cc,
                                  const float* wp, float* psfc, const float* lo, const float* di, const float* up,
                                  void* stream);

/* ---- 3r. Relaxation of a resident plan's tracers to a level profile, in place (Newtonian relaxation, the last per-step
 * operator of a host model that forced f out of a plan: SAM's damping layer under the model top, t(i,k) = t(i,k) -
 * dtn * tau(k) * (t(i,k) - t0(k)) with t0 the horizontal mean of the field itself, and nudging towards a given profile.
 * The update scales each cell's deviation, so it is no per-level increment (3i), and 3p could apply it only from a
 * per-cell array the caller would have to form from f).  This section is the specification; the reference tree has no
 * such routine.  For instance sl in [sl0, sl0 + n), tracer t in [first_tracer, first_tracer + ntracers), level
 * k = 1 .. nzm, nzm = nz - 1, interior column i = 1 .. nx, with b = sl - sl0:
 *   target == NULL :  s = +0;  do i = 1, nx:  s = s + f_old(sl,i,k,t)        (the sum of 3g, in that order)
 *                     m = s / nx                                             (nx converted exactly; ONE divide)
 *   target != NULL :  m = target(b,k,t)
 *   mean(b,k,t) = m                                                          (NULL: skipped; written in both modes)
 *   c(b,k) == 0 (either sign):  f(sl,:,k,t) keeps every bit -- the level is not rewritten
 *   else, per i:      d = f_old(sl,i,k,t) - m;  p = c(b,k) * d;  f(sl,i,k,t) = f_old(sl,i,k,t) - p
 * Every operation is rounded ONCE in the plan's precision, in exactly this association; nothing is contracted, so EXACT
 * and FAST plans give the same bits.  The divide is the IEEE one, correctly rounded in both precisions: on an fp32 plan
 * m is NOT float(double(s) / nx) and not s times a rounded reciprocal.  NaN and infinities are outside the contract.
 * c = 1 does not make the field uniform bit for bit: f - (f - m) is m only up to the two roundings.
 * All arrays are of the plan's precision, reference layout, instance index fastest, leading dimension n (the block's
 * first instance at index 0), tightly packed, tracer slowest:
 *   c      (n, nzm)                shared by the columns and the tracers, as 3o shares its coefficients; required, only read
 *   target (n, nzm [, ntracers])   only read; may be NULL (relax to the horizontal mean)
 *   mean   (n, nzm [, ntracers])   only written; may be NULL
 * No byte outside these arrays is read or written.  Afterwards the plan behaves exactly as if the interior of f had been
 * exported, changed as above and imported again.
 * Towards the rest of a plan:
 *   halo marks   only interior columns are read and written; halo columns are neither.  GIVEN plans: halos keep every
 *     bit.  PERIODIC plans: no wrap is launched, because the mean is taken over the interior alone; the halo marks of the
 *     range are cleared afterwards, so the next run or read-back hands out wrapped halos of the new field.
 *   windowed plans (3e, nz > 238) are supported.  Given m the operator is pointwise in k, and m is the sum of the level's
 *     own interior columns, so no seam refresh is needed in front: an owned level is right whatever the seams hold (as
 *     3k argues).  The scheme chosen: the call reads and writes OWNED levels only, each with c and the target of the tall
 *     level it stands for, and clears the seam marks of the range afterwards; the next run refreshes the other copies,
 *     whether the seams were fresh or stale at the call.  mean of a level is written by that level's owner.  c, target
 *     and mean are addressed by tall level directly in the caller's arrays: nothing is cut into windows.
 *   odd fp32 plans (3f)  the phantom half follows instance ncrms - 1 whenever the block holds it (on a windowed plan the
 *     phantom of the inner plan is restored behind the call, as in 3m / 3n / 3p).
 *   untouched    an fp32 block that splits a pair stores the partner back as loaded: a -0.0 there stays; padding slots,
 *     neighbours in a tile, instances and tracers outside the ranges, flux, u, w, rho, rhow, adz, the held-velocity
 *     flags, the boundary mode and the timing pair keep every bit.  The call is outside the run's event pair; the plan
 *     need not hold velocities.
 * A kernel of its own on every kind of plan (mpdata_relax.hip), not fused into the run.  Wave-major and windowed plans: a
 * lane owns one (instance, level) element and walks its interior column slots (the walk of 3g and 3i), so the horizontal
 * sum is lane-local: no LDS, no barrier, no cross-lane traffic, and no ordering to argue -- a lane touches the columns of
 * its own element only.  With a target: ONE walk that loads and stores f, m and c in registers; a wave whose elements
 * all have c == 0 loads nothing.  Without one, two forms: nx <= 32, the KEPT form -- the nx columns of
 * the lane's element are loaded into registers once (64 registers at nx = 32, fully unrolled, no scratch), summed,
 * updated and stored, so f is read from HBM once; nx > 32, the RE-READ form -- the summing walk of 3g, the divide, then
 * the updating walk over the same columns; that its second read of f is served by L2 is a supposition: not counted.
 * Both forms give the same bits.  Reference-layout plans and the array forms: one thread per instance and (level,
 * tracer) row, two loops over i, in place, no scratch array.
 * Checked before any device call, in this order -- a failed call changes nothing:
 * MPDATA_EINVAL: null plan, n < 1, a range outside [0, ncrms), a bad tracer range, a null c; in the array forms bad sizes
 * (ncrms < 1, nx < 1, nz < 2, ntracers < 1), a block outside the arrays, a null f, then a null c.
 * MPDATA_EUNSUPPORTED: a multi-GPU handle, as in 3d - 3q (take mpdata_plan_shard_plan(plan, g) and a shard-local sl0).
 * MPDATA_ESTATE: a host form of the other precision; a plan never filled.
 * Time on the MI355X (docs/EXPERIMENTS.md Y, tools/relax_bench.py, profiles/relax_bench.json), 65536 x 32 x 28, one tracer,
 * cold: to the mean 0.203 ms fp64, 0.102 ms fp32; to a target 0.205 / 0.109 ms -- 4.5 / 4.4 and 4.4 / 4.1 TB/s of the
 * algorithmic bytes (the interior of f read once and written once: 2 nx nzm ncrms reals, 0.906 GB fp64).  Against existing
 * calls in the same run, mean mode / target mode: (a) 0.47 x / 0.48 x fp64 and 0.46 x / 0.49 x fp32
 * mpdata_plan_export_device + mpdata_plan_import_device of f alone (the old route without the caller's kernel); (b) 0.59 x /
 * 0.60 x and 0.61 x / 0.65 x mpdata_plan_level_stats_device (sum) + mpdata_plan_level_add_device; (c) 0.90 x / 0.90 x and
 * 0.88 x / 0.94 x mpdata_plan_level_add_device alone.  With 25 tracers: 5.49 / 5.55 ms fp64, 2.62 / 2.75 ms fp32 (0.54 x (a),
 * 0.62 x (b), 0.84 x (c) in fp64).  Tall plans, 4096 x 32 x 300 (6 windows): 0.147 / 0.154 ms fp64, 0.078 / 0.086 ms fp32,
 * 0.39 x / 0.41 x (a), 0.59 x / 0.61 x (b), 0.91 x / 0.95 x (c) in fp64.  The KEPT form against the RE-READ form at the same
 * shapes: 0.203 against 0.224 ms fp64, 0.102 / 0.117 fp32, 0.147 / 0.181 and 0.078 / 0.095 tall -- 7 % to 19 %, where three
 * runs of one form differ by 3 % at most; with 25 tracers in fp64 no gain beyond that spread.  Said plainly: both modes are
 * below (c) only because they move 32 of its 38 columns; per byte neither reaches level_add's rate (4.7 TB/s), and target
 * mode, with 8 loads in flight per lane where the kept form has 32, is the slower of the two although it does less. */
/* instances [sl0, sl0+n) of a resident plan; whole plan: sl0 = 0, n = ncrms.  Device arrays of the plan's precision on
 * the plan's device, asynchronous on the plan's stream. */
int mpdata_plan_relax_device(mpdata_plan* plan, int64_t sl0, int64_t n, const void* c, const void* target, void* mean,
                             int first_tracer, int ntracers);
/* host arrays, all tracers, synchronous (the plan's block staging buffer, as the 3g - 3q host forms) */
int mpdata_plan_relax(mpdata_plan* plan, int64_t sl0, int64_t n, const double* c, const double* target, double* mean);
int mpdata_plan_relax_f32(mpdata_plan* plan, int64_t sl0, int64_t n, const float* c, const float* target, float* mean);
/* the same on instances [sl0, sl0+n) of a reference-layout DEVICE array f(ncrms,-2:nx+3,1,nzm[,ntracers]) (leading
 * dimension ncrms); c, target, mean as above (leading dimension n).  Asynchronous on `stream`; 64-bit offsets. */
int mpdata_relax_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, double* f, const double* c,
                        const double* target, double* mean, void* stream);
int mpdata_relax_f32_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, float* f, const float* c,
                            const float* target, float* mean, void* stream);

/* ---- 3s. Implicit vertical diffusion of a resident plan's tracers with a per-cell diffusivity, in place (the implicit half
 * of 3l: SAM's eddy diffusivity tkh differs in every cell, large in clouds and near zero beside them, so 3o, whose matrix is
 * one per instance, cannot take it, and 3l, which can, is explicit and bound by cz * tkh <= 1/2 on thin layers).  The call
 * takes the SAME tkh array 3l takes and the same cz, forms the tridiagonal matrix of every column from them and solves it
 * where f lies: mpdata_plan_diffuse_device with cz = 0 followed by this call is an x-explicit, z-implicit diffusion step
 * without f leaving the plan.  This section is the specification; the reference tree has no such routine.  For instance sl
 * in [sl0, sl0 + n), tracer t in [first_tracer, first_tracer + ntracers), interior column i = 1 .. nx, nzm = nz - 1, each
 * statement one rounded operation in the plan's precision, nothing contracted, the divide IEEE, every f on the right-hand
 * side the value BEFORE the call:
 *   ir(k)   = 1 / (rho(sl,k) * adz(sl,k))                        (the plan's rho, adz; as 3l)
 *   s       = tkh(sl,i,k) + tkh(sl,i,k+1);  e(i,k) = cz(sl,k) * s     k = 1 .. nzm-1     (the product inside 3l's Fz)
 *   e(i,0)  = e(i,nzm) = +0
 *   a(k)    = e(i,k-1) * ir(k);   c(k) = e(i,k) * ir(k);   t = 1 + a(k);   di(k) = t + c(k)
 *   r(k)    = f(i,k),  except  r(1) = f(i,1) + sb(sl,i) * ir(1)   and   r(nzm) = f(i,nzm) - st(sl,i) * ir(nzm)
 *             (a NULL sb / st skips its statement; nzm = 1: first the sb statement, then st on its result)
 *   forward:  p = 1 / di(1);  g(1) = c(1) * p;  y(1) = r(1) * p
 *             k = 2 .. nzm:  m = a(k) * g(k-1);  d = di(k) - m;  p = 1 / d;  g(k) = c(k) * p
 *                            q = a(k) * y(k-1);  v = r(k) + q;   y(k) = v * p
 *   backward: x(nzm) = y(nzm);   k = nzm-1 .. 1:  m = g(k) * x(k+1);  x(k) = y(k) + m
 *   f(i,k) = x(k)
 * This is backward Euler of 3l's vertical part, x - f = -(Fz(k) - Fz(k-1)) * ir(k) with Fz taken from x, solved by the
 * Thomas recurrence without PIVOTING.  The matrix is diagonally dominant for every cz, tkh >= 0 (row sums 1, non-positive
 * off-diagonals: the discrete maximum principle holds in exact arithmetic).  The library looks at no sign.
 * All arrays are of the plan's precision, reference layout, instance index fastest, leading dimension n (the block's first
 * instance at index 0), tightly packed:
 *   tkh   (n, 0:nx+1, nzm)     3l's array as it is, shared by the tracers; columns 0 and nx+1 are never read
 *   cz    (n, nzm)             3l's meaning and SAM folding, 0.5 dtn grdf_z(k) / dz^2 * rhow(k+1) / adzw(k+1), the 0.5 that
 *                              of the mean (tkh(k) + tkh(k+1)) / 2 and dtn the FULL step of the implicit solve: a caller
 *                              that sub-cycles 3l (dtn / ncycle, to keep cz * tkh <= 1/2) does not apply the factor of
 *                              its explicit sub-step here; cz(:, nzm) is never read
 *   sb,st (n, nx)              the scaled surface and top fluxes, 3l's sign convention; either may be NULL
 * Relation to 3o: where tkh does not depend on i the result is, bit for bit, mpdata_plan_vsolve_device with lo = -a, di,
 * up = -c -- negation is exact, and the statements above are 3o's with the signs folded (m = lo * g(k-1) = a * g there as here,
 * r = f - lo * y = f + a * y, x = y - g3o * x = y + g * x).
 * Identity: tkh = 0 (or cz = 0) with NULL sb, st keeps every bit of f, except that a -0.0 may come back as +0.0: a = c = +0,
 * di = 1, p = 1, g = +0, so q = +0 * y(k-1) and m = +0 * x(k+1) are zeros whose sign is that of the neighbour, and
 * -0.0 + +0.0 = +0.0.  (sb or st given as arrays of +0 do the same to level 1 and nzm: f + +0.0.)
 * Contract: NaN, infinities and a zero pivot are outside the contract.  EXACT and FAST plans give the same bits.
 * Towards the rest of a plan:
 *   halo marks   only interior columns are read or written.  No wrap is launched before the call, because nothing couples
 *     in x.  GIVEN plans: halos keep every bit.  PERIODIC plans: the halo marks of the range are cleared afterwards, so the
 *     next run or read-back hands out wrapped halos of the new field.
 *   odd fp32 plans (3f)  the phantom half follows instance ncrms - 1 whenever the block holds it.
 *   untouched    an fp32 block that splits a pair stores the partner back as loaded; padding slots, neighbours in a group,
 *     instances and tracers outside the ranges, flux, u, w, rho, rhow, adz, the held-velocity flags, the boundary mode and
 *     the timing pair keep every bit.  The call is outside the run's event pair; the plan need not hold velocities.
 *   windowed plans (3e, nz > 238): MPDATA_EUNSUPPORTED.  The backward sweep needs g of every cell of the windows below,
 *     so a second pass would have to park g in device memory; 3l, the other half of the pair, refuses such plans too.
 *     The named follow-up, not built yet.
 * No zflux output: take the tendency from mpdata_plan_level_stats_device before and after, as 3o says.
 * Kernels of their own on every kind of plan (mpdata_vdiffuse.hip), not fused into the run.  A small kernel in front forms
 * ir once per call (n nzm reals in the plan's diffusion buffer of 3l).  Wave-major plans: the geometry of 3o -- a
 * workgroup stages the column slots of 16 adjacent 8-byte elements of the instance axis (fewer where the levels would not
 * fit) and a batch of columns through LDS, and beside them the rows of tkh of those instances and columns, read where they
 * lie as 3n reads wp, and cz and ir per (element, level); a lane per (instance element, column) sweeps up and down in LDS in
 * place, g(k) overwriting tkh(k) once e(k) is formed, so a cell takes two LDS elements and a batch is 4 columns at 27
 * levels where 3o's is 8; the waves store LDS back to f as the same linear streams.  Every global load precedes a barrier
 * and every global store follows the sweeps' barrier; workgroups own disjoint elements: the in-place update is race-free
 * by construction.  The tracers of a call are workgroups of one launch, each forming the factors again (the form that
 * keeps them in LDS across the tracers was not built: docs/EXPERIMENTS.md AC).  Reference-layout plans and the array forms:
 * one thread per instance and column sweeps its column in place, tracer after tracer, g in a scratch array (n nx nzm reals:
 * the plan's diffusion buffer; an allocation of the call's own in the array forms).
 * Checked before any device call, in this order -- a failed call changes nothing:
 * MPDATA_EINVAL: null plan, n < 1, a range outside [0, ncrms), a bad tracer range, a null tkh or cz; in the array forms bad
 * sizes (ncrms < 1, nx < 1, nz < 2, ntracers < 1), a block outside the arrays, a null f, rho or adz, then a null tkh or cz.
 * MPDATA_EUNSUPPORTED: a multi-GPU handle, as in 3d - 3r (take mpdata_plan_shard_plan(plan, g) and a shard-local sl0); a
 * windowed plan.  MPDATA_ESTATE: a host form of the other precision; a plan never filled.  mpdata_last_error names the
 * argument.
 * Time on the MI355X (docs/EXPERIMENTS.md AC, tools/vdiffuse_bench.py, profiles/vdiffuse_bench.json), 65536 x 32 x 28, one tracer,
 * cold: 0.515 ms fp64, 0.297 ms fp32 (the ir kernel included) -- 2.6 / 2.3 TB/s of the algorithmic bytes (the interior of f read
 * once and written once, the interior of tkh read once: 3 nx nzm ncrms reals, 1.36 GB fp64); three batches differ by 2.1 % at
 * most.  Against the parent's calls in the same run: 1.22 x / 1.27 x mpdata_plan_export_device + mpdata_plan_import_device of
 * f alone (the old route without the caller's kernel), 1.97 x / 1.79 x mpdata_plan_vsolve_device (the same sweep, no per-cell
 * field, no divide in the hot kernel), 1.65 x / 1.83 x mpdata_plan_sediment_device (the same algorithmic bytes), 1.03 x /
 * 1.17 x mpdata_plan_diffuse_device (the full 3l).  25 tracers: 11.73 / 6.50 ms, 1.14 x / 1.25 x the export + import.  A block of
 * 64 instances: 0.016 ms.  4096 x 32 x 238: 1.51 / 1.01 ms, 4.8 x / 6.2 x the export + import (4 of 256 lanes sweep there).
 * Said plainly: the call does NOT beat the export + import of f at any shape measured.  It is bound by the sweep -- one wave
 * of four carries a dependent chain with an IEEE divide per level, 64 of 256 lanes at work -- not by its bytes, which
 * sediment moves in 0.61 of the time.  What it saves is the caller's tridiagonal kernel behind that export, the sub-cycling
 * of 3l on thin layers and the host-side bookkeeping.  A 48 KiB and a 64 KiB LDS budget of the kernel's own
 * were timed against the 40 KiB kept: 8 % slower at 28 levels. */
/* instances [sl0, sl0+n) of a resident plan; whole plan: sl0 = 0, n = ncrms.  Device arrays of the plan's precision on
 * the plan's device, asynchronous on the plan's stream. */
int mpdata_plan_vdiffuse_device(mpdata_plan* plan, int64_t sl0, int64_t n, const void* tkh, const void* cz, const void* sb,
                                const void* st, int first_tracer, int ntracers);
/* host arrays, all tracers, synchronous (the plan's block staging buffer, as the 3g - 3r host forms) */
int mpdata_plan_vdiffuse(mpdata_plan* plan, int64_t sl0, int64_t n, const double* tkh, const double* cz, const double* sb,
                         const double* st);
int mpdata_plan_vdiffuse_f32(mpdata_plan* plan, int64_t sl0, int64_t n, const float* tkh, const float* cz, const float* sb,
                             const float* st);
/* the same on instances [sl0, sl0+n) of reference-layout DEVICE arrays f(ncrms,-2:nx+3,1,nzm[,ntracers]), rho(ncrms,nzm),
 * adz(ncrms,nzm) (leading dimension ncrms); tkh, cz, sb, st as above (leading dimension n).  Enqueued on `stream`; the call
 * allocates its scratch array and returns when the work is done and the scratch is freed. */
int mpdata_vdiffuse_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, double* f, const double* rho,
                           const double* adz, const double* tkh, const double* cz, const double* sb, const double* st,
                           void* stream);
int mpdata_vdiffuse_f32_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, float* f, const float* rho,
                               const float* adz, const float* tkh, const float* cz, const float* sb, const float* st,
                               void* stream);

/* ---- 3t. First-order conversion between two tracers of a resident plan, in place (the one piece of a cloud model's scalar
 * step that couples two species of the same cell: autoconversion of cloud water into rain, d = r * max(qc - qc0, 0), taken
 * from one species and given to the other; ageing and decay chains of passive tracers; a first-order chemical loss with a
 * yield; a phase change with its latent-heat increment on a temperature-like tracer.  Every call of 3g - 3s works on one
 * tracer at a time; this one sees two).  This section is the specification; the reference tree has no such routine.  For one
 * ordered pair of tracers (src, dst), every instance sl in [sl0, sl0 + n) with b = sl - sl0, every level k = 1 .. nzm,
 * nzm = nz - 1, and every INTERIOR column i = 1 .. nx, with a = f_old(i,k,src) and c = f_old(i,k,dst), every statement
 * below is rounded once in the plan's precision, in this association, with no contraction; comparisons are plain
 * compare-and-select, never fmax / fmin:
 *   r(b,k) == 0            : the level keeps every bit in BOTH tracers and is not stored; dsum(b,k) = +0
 *   e = q0 ? a - q0(b,k) : a
 *   e = (e > 0) ? e : +0                       (so NaN and -0 give +0)
 *   d = r(b,k) * e
 *   mode & MPDATA_CONVERT_LIMIT:  m = (a > 0) ? a : +0 ;  d = (d > m) ? m : d
 *   f(i,k,src) = a - d
 *   g = y ? y(b,k) * d : d
 *   f(i,k,dst) = c + g
 *   dsum(b,k): s = +0; do i = 1, nx: s = s + d(i)        (NULL: skipped)
 * r (required), q0, y (optional inputs, NULL: absent) and dsum (optional output) are (n, nzm) arrays of the plan's
 * precision, reference layout, instance index fastest, leading dimension n (the block's first instance at index 0), as c of
 * 3r.  r may have either sign; LIMIT caps d from above only (with r in [0, 1] and a >= q0 >= 0 it never bites; it is for
 * r * dt > 1, where src would go negative); a reverse conversion swaps src and dst.  Halo columns are neither read nor
 * written.  A tracer that is neither src nor dst keeps every bit.  EXACT and FAST plans give the same bits.  With y == NULL
 * the amount added to dst is the amount taken from src, so src + dst is conserved up to the two roundings of a - d and
 * c + d.  No byte outside the arrays is read or written.  Afterwards the plan behaves exactly as if the interior of the two
 * tracers had been exported, changed as above and imported again.
 * Towards the rest of a plan:
 *   halo marks   only interior columns are read and written.  GIVEN plans: halos keep every bit.  PERIODIC plans: no wrap
 *     is launched; the halo marks of BOTH tracers are cleared afterwards, so the next run or read-back hands out wrapped
 *     halos of the new fields.
 *   windowed plans (3e, nz > 238) are supported, as in 3r: the operator is pointwise, the call reads and writes OWNED levels
 *     only, each with r, q0 and y of the tall level it stands for, needs no seam refresh in front and clears the seam marks
 *     of both tracers afterwards; dsum of a level is written by that level's owner.
 *   odd fp32 plans (3f)  the phantom half follows instance ncrms - 1 in both tracers whenever the block holds it and its r
 *     is not zero on that level (on a windowed plan the phantom of the inner plan is restored behind the call, as in 3r).
 *   untouched    an fp32 block that splits a pair stores the partner back as loaded: a -0.0 there stays; padding slots,
 *     neighbours in a tile, instances outside the block, every other tracer, flux, u, w, rho, rhow, adz, the held-velocity
 *     flags, the boundary mode and the timing pair keep every bit.  The call is outside the run's event pair; the plan need
 *     not hold velocities.
 * A kernel of its own on every kind of plan (mpdata_convert.hip), not fused into the run.  Wave-major and windowed plans: a
 * lane owns one (instance, level) element and walks its interior column slots as TWO linear streams (the walk of 3g and 3i),
 * 8 columns in flight on each: the src tracer and, at a signed 64-bit offset from it, the dst tracer.  r, q0 and y are in
 * registers, dsum is lane-local in column order: no LDS, no barrier, no cross-lane traffic, and no ordering to argue -- a
 * lane touches the columns of its own element only, in two tracers.  A wave whose elements all have r == 0 loads nothing.
 * Reference-layout plans and the array forms: one thread per instance and level row, one loop over i, in place.
 * Checked before any device call, in this order -- a failed call changes nothing:
 * MPDATA_EINVAL: null plan, n < 1, a range outside [0, ncrms), src or dst outside [0, ntracers), src == dst, a null r, a
 * mode bit other than MPDATA_CONVERT_LIMIT; in the array forms bad sizes (ncrms < 1, nx < 1, nz < 2, ntracers < 1), a block
 * outside the arrays, a null f, then the pair, r and the mode as above.
 * MPDATA_EUNSUPPORTED: a multi-GPU handle, as in 3d - 3s (take mpdata_plan_shard_plan(plan, g) and a shard-local sl0).
 * MPDATA_ESTATE: a host form of the other precision; a plan never filled.
 * Time on the MI355X (docs/EXPERIMENTS.md AD, tools/convert_bench.py, profiles/convert_bench.json), 65536 x 32 x 28, cold: with
 * r alone 0.417 ms fp64, 0.210 ms fp32; with q0, y and dsum 0.438 / 0.220 ms -- 4.35 and 4.14 TB/s of the algorithmic bytes (the
 * interior of two tracers read once and written once: 4 nx nzm ncrms reals, 1.81 GB fp64).  Against existing calls in the
 * same run, r alone / with everything: (a) 0.48 x / 0.51 x fp64 and 0.46 x / 0.49 x fp32 mpdata_plan_export_device +
 * mpdata_plan_import_device of both tracers (the old route without the caller's kernel); (b) 0.90 x / 0.94 x and 0.89 x / 0.93 x
 * two mpdata_plan_level_add_device calls; (c) 0.98 x / 1.02 x and 0.96 x / 1.00 x two mpdata_plan_relax_device calls to a target,
 * which move the same bytes.  LIMIT and a negative offset (dst < src) cost nothing.  A block of 64 instances: 0.007 ms.  Tall
 * plans, 4096 x 32 x 300 (6 windows): 0.299 / 0.318 ms fp64, 0.157 / 0.174 ms fp32, 0.41 x / 0.44 x (a) in fp64.  Said plainly: per
 * byte the call does not reach level_add's rate (4.35 against 4.62 TB/s) and sits at relax's, whose interior-only walk it
 * shares.  NB = 4 on both streams (8 waves per SIMD where NB = 8 has 5) was timed against it: 1.3 % to 1.6 % slower. */
#define MPDATA_CONVERT_LIMIT 1 /* mode bit: cap d from above by max(a, 0), so that src does not change sign */
/* instances [sl0, sl0+n) of a resident plan; whole plan: sl0 = 0, n = ncrms.  Device arrays of the plan's precision on
 * the plan's device, asynchronous on the plan's stream. */
int mpdata_plan_convert_device(mpdata_plan* plan, int64_t sl0, int64_t n, int src, int dst, const void* r, const void* q0,
                               const void* y, int mode, void* dsum);
/* host arrays, synchronous (the plan's block staging buffer, as the 3g - 3s host forms) */
int mpdata_plan_convert(mpdata_plan* plan, int64_t sl0, int64_t n, int src, int dst, const double* r, const double* q0,
                        const double* y, int mode, double* dsum);
int mpdata_plan_convert_f32(mpdata_plan* plan, int64_t sl0, int64_t n, int src, int dst, const float* r, const float* q0,
                            const float* y, int mode, float* dsum);
/* the same on instances [sl0, sl0+n) of a reference-layout DEVICE array f(ncrms,-2:nx+3,1,nzm,ntracers) (leading
 * dimension ncrms); r, q0, y, dsum as above (leading dimension n).  Asynchronous on `stream`; 64-bit offsets. */
int mpdata_convert_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, double* f, int src, int dst,
                          const double* r, const double* q0, const double* y, int mode, double* dsum, void* stream);
int mpdata_convert_f32_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, float* f, int src, int dst,
                              const float* r, const float* q0, const float* y, int mode, float* dsum, void* stream);

/* ---- 3u. Per-level covariance of two tracers of a resident plan (the read side of a cloud model's second moments: the
 * horizontal variance of a tracer per level, the covariance of two, the amplitude that variance transport in a multiscale
 * modelling framework hands to the global model, SAM-style statistics such as QT2 and TL2.  3g gives first moments and
 * extrema, 3k column integrals; everything that needs a product of deviations forced f out of the plan.  The feedback of
 * variance transport -- scaling each cell's deviation from the level mean -- is mpdata_plan_relax_device (3r) in mean mode
 * with c = 1 - factor: only the diagnosis was missing).  This section is the specification; the reference tree has no such
 * routine.  For one pair of tracers (ta, tb) -- ta == tb is allowed and gives the variance --, every instance sl in
 * [sl0, sl0 + n) with b = sl - sl0, every level k = 1 .. nzm, nzm = nz - 1, over the INTERIOR columns i = 1 .. nx, with
 * a_i = f(sl,i,k,ta) and b_i = f(sl,i,k,tb), every statement below is rounded ONCE in the plan's precision, in this
 * association, with nothing contracted, so EXACT and FAST plans give the same bits:
 *   mode & MPDATA_LEVEL_COV_RAW :  da_i = a_i ;  db_i = b_i                  (no subtraction at all)
 *   otherwise:
 *       m_a = ma ? ma(b,k) : ( s = +0; do i = 1, nx: s = s + a_i ;  s / nx )   (the sum of 3g, ONE IEEE divide, as 3r)
 *       m_b = mb ? mb(b,k) : the same from b_i
 *       mean_a(b,k) = m_a ;  mean_b(b,k) = m_b                               (NULL: skipped; written in both cases)
 *       da_i = a_i - m_a ;  db_i = b_i - m_b
 *   c = +0;  do i = 1, nx:  p = da_i * db_i ;  c = c + p
 *   cov(b,k) = c
 * cov is the SUM over the columns, not divided by nx and not by nx - 1: the caller normalises, as with sum of 3g, so no
 * rounding is hidden.  The two-pass form is the definition; the one-pass form  sum(a b) - sum(a) sum(b) / nx  is not, and
 * differs from it in bits in most outputs.  The divide is the correctly rounded IEEE one in both precisions, not a product
 * with a rounded reciprocal (on random fields more than a fifth, a tenth and a thirtieth of the outputs differ at nx = 3,
 * 11 and 17).  NaN and infinities are outside the contract.  ma, mb (optional inputs), cov (required output), mean_a, mean_b (optional outputs)
 * are (n, nzm) arrays of the plan's precision, reference layout, instance index fastest, leading dimension n (the block's
 * first instance at index 0), as c of 3r.  With ta == tb, ma and mb may still differ; the definition above covers it.
 * Towards the rest of a plan, exactly as 3g: halo columns are never read, so a PERIODIC plan needs no wrap; nothing of the
 * plan's state changes -- filled, have_u, have_w, the halo marks, the seam marks, the timing pair and last_kernel_ms --;
 * the call is outside the run's event pair; the plan need not hold velocities.
 *   windowed plans (3e, nz > 238) are supported: only OWNED levels are read, each is written to the tall level it stands
 *     for and uses ma / mb of that tall level, and no seam refresh is launched in front.
 *   no output is reached by the phantom half of an odd fp32 plan (3f), the partner of a split fp32 pair or a padding slot,
 *     and no byte outside the five arrays is touched.
 * A kernel of its own on every kind of plan (mpdata_level_cov.hip), not fused into the run.  Wave-major and windowed plans:
 * a lane owns one (instance, level) element and walks its interior column slots as two read-only linear streams (the walk
 * of 3t), 8 columns in flight on each: tracer ta and, at a signed 64-bit offset from it, tracer tb; with ta == tb ONE
 * stream.  No LDS, no barrier, no cross-lane traffic.  Three forms with the same bits: ONE-PASS (RAW, or both profiles
 * given), KEPT (a mean is formed and nx <= 32: the columns stay in registers between the two passes, so f is read once) and
 * RE-READ (a mean is formed, nx > 32: the summing walk of 3g, the divides, then the accumulating walk).  A wave none of
 * whose elements is in the block, or owned in a window, loads nothing.  Reference-layout plans and the array forms: one
 * thread per instance and level row, loops over i, 64-bit offsets.
 * Checked before any device call, in this order -- a failed call changes nothing:
 * MPDATA_EINVAL: null plan, n < 1, a range outside [0, ncrms), ta or tb outside [0, ntracers), a mode bit other than
 * MPDATA_LEVEL_COV_RAW, RAW together with a non-null ma, mb, mean_a or mean_b, a null cov; in the array forms bad sizes
 * (ncrms < 1, nx < 1, nz < 2, ntracers < 1), a block outside the arrays, a null f, then the same list as above.
 * MPDATA_EUNSUPPORTED: a multi-GPU handle, as in 3d - 3t (take mpdata_plan_shard_plan(plan, g) and a shard-local sl0).
 * MPDATA_ESTATE: a host form of the other precision; a plan never filled.
 * Time on the MI355X (docs/EXPERIMENTS.md AE, tools/level_cov_bench.py, profiles/level_cov_bench.json), 65536 x 32 x 28,
 * cold, ta != tb, fp64 / fp32: both means formed (the kept form) 0.174 / 0.092 ms -- 5.2 / 5.0 TB/s of the algorithmic bytes
 * (the interior of two tracers read once: 2 nx nzm ncrms reals, 0.91 GB fp64; one tracer for ta == tb) --, with mean_a and
 * mean_b written 0.200 / 0.108, RAW 0.180 / 0.089, both profiles given 0.187 / 0.098; ta == tb: 0.093 / 0.047 formed, 0.096 /
 * 0.051 RAW.  Against existing calls in the same run, means formed: (a) 0.42 x / 0.42 x mpdata_plan_export_device of the two
 * tracers (0.418 / 0.219 ms: the old route without the caller's kernel); (b) 0.91 x / 0.91 x two mpdata_plan_level_stats_device
 * calls (0.190 / 0.100 ms), which read the same bytes once without the products.  A negative offset (tb < ta) costs nothing.
 * A block of 64 instances: 0.006 ms.  Tall plans, 4096 x 32 x 300 (6 windows): 0.139 / 0.080 ms formed, 0.42 x / 0.28 x (a),
 * 0.93 x / 0.86 x (b).  The kept form against the re-read form at nx = 32 (the same library with the kept limits at 0, same
 * session): two tracers 0.174 against 0.255 ms fp64 and 0.092 against 0.137 fp32 (146 and 206 VGPRs, 3 and 2 waves per SIMD,
 * no scratch, no spill), one tracer 0.093 against 0.128 and 0.047 against 0.070 (82 VGPRs): kept wins by 27 % to 33 %, far
 * beyond the 3 % run-to-run spread of 3r, at 28 and at 300 levels, so both kept forms stay at nx <= 32.  Said plainly: above
 * nx = 32 the re-read form is what runs, and it LOSES to two level_stats calls (1.33 x fp64, 1.38 x fp32; still 0.63 x / 0.65 x
 * the export): its second read costs a third of a first read, so the caches serve part of it, not all.  Writing the two
 * means costs 15 % -- the outputs of a wave lie a leading dimension apart, as those of 3g -- and the given-profile call is
 * 7 % to 10 % slower than forming the means in the kept form, which has all its loads in flight at once. */
#define MPDATA_LEVEL_COV_RAW 1 /* mode bit: the sum of a_i * b_i, no mean subtracted; ma, mb, mean_a, mean_b must be NULL */
/* instances [sl0, sl0+n) of a resident plan; whole plan: sl0 = 0, n = ncrms.  Device arrays of the plan's precision on
 * the plan's device, asynchronous on the plan's stream. */
int mpdata_plan_level_cov_device(mpdata_plan* plan, int64_t sl0, int64_t n, int ta, int tb, const void* ma, const void* mb,
                                 int mode, void* cov, void* mean_a, void* mean_b);
/* host arrays, synchronous (the plan's block staging buffer, as the 3g - 3t host forms) */
int mpdata_plan_level_cov(mpdata_plan* plan, int64_t sl0, int64_t n, int ta, int tb, const double* ma, const double* mb,
                          int mode, double* cov, double* mean_a, double* mean_b);
int mpdata_plan_level_cov_f32(mpdata_plan* plan, int64_t sl0, int64_t n, int ta, int tb, const float* ma, const float* mb,
                              int mode, float* cov, float* mean_a, float* mean_b);
/* the same on instances [sl0, sl0+n) of a reference-layout DEVICE array f(ncrms,-2:nx+3,1,nzm,ntracers) (leading
 * dimension ncrms), which is only read; ma, mb, cov, mean_a, mean_b as above (leading dimension n).  Asynchronous on
 * `stream`; 64-bit offsets. */
int mpdata_level_cov_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, const double* f, int ta, int tb,
                            const double* ma, const double* mb, int mode, double* cov, double* mean_a, double* mean_b,
                            void* stream);
int mpdata_level_cov_f32_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, const float* f, int ta,
                                int tb, const float* ma, const float* mb, int mode, float* cov, float* mean_a, float* mean_b,
                                void* stream);

/* ---- 3v. Per-level conditional counts and sums of a resident plan's tracers (the third kind of horizontal statistic a
 * host model takes from its CRM instances every step, next to the first moments and extrema of 3g and the second moments
 * of 3u: the share of the columns of a level in which a tracer exceeds a threshold, and the sum of other tracers over
 * exactly those columns -- the cloud fraction profile handed to the radiation of the global model, in-cloud means of the
 * water species, "core" and "environment" averages, a histogram of a tracer per level taken bin by bin.  The minimum and
 * maximum of 3g only say whether ANY column is in; everything else forced the condition tracer and every sampled tracer
 * out of the plan).  This section is the specification; the reference tree has no such routine.  For one condition
 * tracer tc, a range of value tracers [first_tracer, first_tracer + ntracers) -- tc may lie inside it --, every instance
 * sl in [sl0, sl0 + n) with b = sl - sl0, every level k = 1 .. nzm, nzm = nz - 1, over the INTERIOR columns i = 1 .. nx,
 * with c_i = f(sl,i,k,tc) and v_i = f(sl,i,k,t), every statement below is rounded ONCE in the plan's precision, in this
 * association, with nothing contracted, and the comparisons are plain compare-and-select, so EXACT and FAST plans give
 * the same bits:
 *   in_i = (lo ? c_i >  lo(b,k) : true)  and  (hi ? c_i <= hi(b,k) : true)     (half-open: bins (lo, hi] tile the line)
 *   cnt(b,k)    :  q = +0;  do i = 1, nx:  if in_i:  q = q + 1                 (a real of the plan's precision; NULL: skipped)
 *   csum(b,k,j) :  s = +0;  do i = 1, nx:  if in_i:  s = s + v_i               (j = t - first_tracer; NULL: skipped)
 * The interval is half-open, (lo, hi]: a column with c_i == lo is out, one with c_i == hi is in, so the bins of a
 * histogram whose edges are each the hi of one bin and the lo of the next count every column exactly once.  Selection
 * means selection: a column that is not in contributes NOTHING, whatever its bits -- an excluded cell of a VALUE tracer
 * may hold an infinity or a NaN and it does not reach csum; multiplying v_i by a 0 / 1 mask is therefore wrong (0 * inf
 * is a NaN).  Adding a selected +0 in place of v_i IS allowed: in round-to-nearest a sum is -0 only when both
 * terms are -0 (an exact zero from terms of opposite sign is +0, and +0 + (-0) = +0), s starts at +0, so by induction s can
 * never be -0, and s + (+0) keeps every bit of every other s.  (cnt likewise: q + (+0) = q.)  NaN in c_i, lo or hi is outside the
 * contract.  lo, hi (optional inputs, at least one required), cnt and csum (optional outputs, at least one required): lo,
 * hi and cnt are (n, nzm) arrays, csum is (n, nzm, ntracers), all of the plan's precision, reference layout, instance
 * index fastest, leading dimension n (the block's first instance at index 0), as sum of 3g.  A level with lo >= hi is
 * empty: cnt = +0, csum = +0.  Sums are SUMS, and cnt is a count: the caller divides (cnt / nx: the fraction; csum / cnt:
 * the conditional mean, where cnt > 0), so no rounding is hidden.  cnt is exact: nx < 2^24.
 * Towards the rest of a plan, exactly as 3g and 3u: halo columns are never read, so a PERIODIC plan needs no wrap; nothing
 * of the plan's state changes -- filled, have_u, have_w, the halo marks, the seam marks, the timing pair and
 * last_kernel_ms --; the call is outside the run's event pair; the plan need not hold velocities.
 *   windowed plans (3e, nz > 238) are supported: only OWNED levels are read, each with lo / hi of the tall level it stands
 *     for, each is written to that tall level, and no seam refresh is launched in front.
 *   no output is reached by the phantom half of an odd fp32 plan (3f), the partner of a split fp32 pair or a padding slot,
 *     and no byte outside cnt and csum is touched.
 * A kernel of its own on every kind of plan (mpdata_level_cond.hip), not fused into the run.  Wave-major and windowed plans:
 * a lane owns one (instance, level) element and walks its interior column slots as read-only linear streams (the walk of
 * 3g / 3u), 8 columns in flight; the value tracers lie at signed 64-bit offsets from the tc stream and are a loop inside
 * the kernel (no tracer axis on the grid); lo and hi sit in registers, every accumulator is lane-local in column order.  No
 * LDS, no barrier, no cross-lane traffic.  Two forms with the same bits: MASK (nx <= 64 and two value tracers or more: one walk over the tc stream forms
 * cnt, the sum of tc under its own condition and a 64-bit in-mask per lane, then one walk per value tracer adds under the
 * mask -- the condition is read ONCE for all tracers, and the walk of t == tc is the first one, kept) and RE-READ (every other call:
 * per value tracer the tc stream and the t stream are walked together, one stream for t == tc, and compared again).  A wave
 * none of whose elements is in the block, or owned in a window, loads nothing.  Reference-layout plans and the array
 * forms: one thread per instance and level row, loops over i, 64-bit offsets.
 * Checked before any device call, in this order -- a failed call changes nothing:
 * MPDATA_EINVAL: null plan, n < 1, a range outside [0, ncrms), tc outside [0, ntracers), lo and hi both NULL, cnt and csum
 * both NULL, with a non-null csum a tracer range that is empty or outside the plan (with csum == NULL the range is not
 * looked at); in the array forms bad sizes (ncrms < 1, nx < 1, nz < 2, ntracers < 1), a block outside the arrays, a null f,
 * then the same list as above.
 * MPDATA_EUNSUPPORTED: a multi-GPU handle, as in 3d - 3u (take mpdata_plan_shard_plan(plan, g) and a shard-local sl0).
 * MPDATA_ESTATE: a host form of the other precision; a plan never filled.
 * Time on the MI355X (docs/EXPERIMENTS.md AF, tools/level_cond_bench.py, profiles/level_cond_bench.json), 65536 x 32 x 28,
 * cold, plans of nine tracers, lo and hi given, 40 % of the columns in, fp64 / fp32: cnt alone 0.103 / 0.060 ms (4.4 / 3.8 TB/s of
 * the algorithmic bytes, the interior of the T + 1 tracers read once: (T + 1) nx nzm ncrms reals); cnt and csum of T = 1, 2, 3,
 * 8 value tracers 0.195 / 0.112, 0.296 / 0.158, 0.378 / 0.225, 0.826 / 0.457 ms -- 4.7 / 4.1, 4.6 / 4.3, 4.8 / 4.0, 4.9 / 4.5 TB/s.  lo alone
 * is 2 % faster.  Against existing calls in the same run: (a) mpdata_plan_export_device of the T + 1 tracers (the old route
 * without the caller's kernel): 0.49 x / 0.51 x for cnt alone, 0.48 x / 0.50 x, 0.49 x / 0.49 x, 0.47 x / 0.53 x, 0.46 x / 0.49 x for T = 1, 2, 3,
 * 8; (b) T + 1 mpdata_plan_level_stats_device calls, which read the same bytes once: 1.12 x / 1.16 x for cnt alone, 1.05 x / 1.10 x,
 * 1.08 x / 1.04 x, 1.04 x / 1.11 x, 1.00 x / 1.01 x.  Said plainly: the call halves the export it replaces and LOSES to the level_stats
 * calls on the same bytes, by 12 % to 16 % for cnt alone and by less the more tracers share the condition -- a compare, a
 * select and, for cnt, a second accumulator per column against one add.  A block of 64 instances: 0.013 / 0.015 ms.  Tall plans,
 * 4096 x 32 x 300 (6 windows), T = 3: 0.325 / 0.192 ms, 0.51 x / 0.34 x (a), 1.07 x / 1.00 x (b).  MASK against RE-READ (the same library
 * with the MASK limit at 0, same session), nx = 32, T = 2, 3, 8: 0.296 against 0.319, 0.378 against 0.448, 0.826 against 1.093 ms fp64
 * (-7 %, -16 %, -24 %), 0.158 / 0.177, 0.225 / 0.252, 0.457 / 0.594 fp32 (-11 %, -11 %, -23 %); nx = 64 (32768 instances): -14 %, -19 %,
 * -27 % fp64 and -15 %, -21 %, -20 % fp32: beyond the 3 % spread of 3r, so MASK runs there.  For cnt alone and for T = 1 both forms
 * read the same bytes and MASK was 6 % SLOWER (cnt alone) or within 4 % either way (T = 1): RE-READ runs for those.  The
 * tracer loop inside the kernel against one call per tracer, which is the traffic of a tracer axis on the grid: 0.378 against
 * 0.557 ms fp64, 0.225 / 0.328 fp32 at T = 3 -- the loop stays. */
/* instances [sl0, sl0+n) of a resident plan; whole plan: sl0 = 0, n = ncrms.  Device arrays of the plan's precision on
 * the plan's device, asynchronous on the plan's stream. */
int mpdata_plan_level_cond_device(mpdata_plan* plan, int64_t sl0, int64_t n, int tc, const void* lo, const void* hi, void* cnt,
                                  void* csum, int first_tracer, int ntracers);
/* host arrays, all tracers (csum (n, nzm, ntracers of the plan)), synchronous (the plan's block staging buffer, as the
 * 3g - 3u host forms) */
int mpdata_plan_level_cond(mpdata_plan* plan, int64_t sl0, int64_t n, int tc, const double* lo, const double* hi, double* cnt,
                           double* csum);
int mpdata_plan_level_cond_f32(mpdata_plan* plan, int64_t sl0, int64_t n, int tc, const float* lo, const float* hi, float* cnt,
                               float* csum);
/* the same on instances [sl0, sl0+n) of a reference-layout DEVICE array f(ncrms,-2:nx+3,1,nzm,ntracers) (leading
 * dimension ncrms), which is only read; lo, hi, cnt, csum as above (leading dimension n; csum (n, nzm, ntr)).  Asynchronous
 * on `stream`; 64-bit offsets. */
int mpdata_level_cond_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, const double* f, int tc,
                             const double* lo, const double* hi, double* cnt, double* csum, int first_tracer, int ntr,
                             void* stream);
int mpdata_level_cond_f32_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, const float* f, int tc,
                                 const float* lo, const float* hi, float* cnt, float* csum, int first_tracer, int ntr,
                                 void* stream);

/* ---- 3w. Per-column conditional level counts, tops and paths of a resident plan's tracers (the column diagnostics a host
 * model takes from its CRM instances every step: shaded cloud cover -- the share of the columns that hold ANY cloudy
 * level, as a whole and in a low, a middle and a high band of levels --, the cloud-base and cloud-top level of every
 * column, and in-cloud water paths, the mass-weighted integral of other tracers over exactly the cloudy levels of a
 * column.  3v answers "how many columns of this level are in"; it cannot answer "is this column in anywhere", which needs
 * the same condition reduced along k per column: this call is the transposed twin of 3v, as 3k is of 3g.  Everything
 * here forced T + 1 tracers out of the plan before).  This section is the specification; the reference tree has no such
 * routine.  For one condition tracer tc, a range of value tracers [first_tracer, first_tracer + ntracers) -- tc may lie
 * inside it --, every instance sl in [sl0, sl0 + n) with b = sl - sl0 and every INTERIOR column i = 1 .. nx, with c_k =
 * f(sl,i,k,tc), v_k = f(sl,i,k,t) and j = t - first_tracer, every statement below is rounded ONCE in the plan's
 * precision, in this association, with nothing contracted, and the comparisons are plain compare-and-select, so EXACT
 * and FAST plans give the same bits:
 *   wgt(sl,k)    = rho(sl,k) * adz(sl,k)                                          (one rounded multiply: 3k's weight)
 *   in_k         = (lo ? c_k >  lo(b,k) : true)  and  (hi ? c_k <= hi(b,k) : true)     (half-open (lo, hi], as 3v)
 *   kcnt(b,i)    :  q = +0;  do k = 1, nzm:  if in_k:  q = q + 1
 *   kbot(b,i)    :  the smallest k in 1 .. nzm with in_k, as a real;  +0 if there is none
 *   ktop(b,i)    :  the largest  k in 1 .. nzm with in_k, as a real;  +0 if there is none
 *   cpath(b,i,j) :  s = +0;  do k = 1, nzm:  if in_k:  s = s + wgt(sl,k) * v_k     (the product rounded, then the add; no fma)
 *   cover(b)     :  q = +0;  do i = 1, nx:   if kcnt(b,i) > 0:  q = q + 1
 *   mass(b,j)    :  s = +0;  do i = 1, nx:   s = s + cpath(b,i,j)                  (3k's mass)
 * lo and hi follow 3v: both optional, at least one required, each an (n, nzm) array of the plan's precision in the
 * reference layout, instance fastest, leading dimension n.  A level with lo >= hi is out in every column, and so is a
 * level with lo = +inf: that is how a caller restricts a call to a BAND of levels per instance (lo = +inf outside the
 * band); three bands -- low, middle, high cloud cover -- are three calls.  Selection means selection: a level that is not in contributes NOTHING,
 * whatever bits an excluded cell of a VALUE tracer holds, an infinity or a NaN included; multiplying by a 0 / 1 mask is
 * therefore wrong (0 * inf is a NaN).  Adding a selected +0 is allowed, by the argument in 3v (s starts at +0 and can
 * never become -0).  NaN in c_k, lo or hi is outside the contract.
 * The six outputs are all optional, at least one is required: kcnt, kbot and ktop are (n, nx) arrays, cpath is (n, nx,
 * ntracers), cover is (n), mass is (n, ntracers); all reals of the plan's precision -- the counts and level indices are
 * exact because nzm, nx < 2^24 --, all in the reference layout with the instance fastest and the tracer slowest, tightly
 * packed, interior columns only.  cover needs kcnt and mass needs cpath (MPDATA_EINVAL otherwise): as in 3k, a second
 * small kernel on the same stream forms them from those arrays.  Without cpath the tracer range is not looked at.
 * Two identities (both tested):  with every level in -- hi = +inf alone, say -- cpath has the bits of 3k's path and mass
 * the bits of its mass;  and sum_i kcnt(b,i) == sum_k cnt(b,k) of 3v for the same tc, lo and hi, both sides exact.
 * Towards the rest of a plan, exactly as 3k and 3v: halo columns are never read, so a PERIODIC plan needs no wrap; nothing
 * of the plan's state changes -- filled, have_u, have_w, the halo marks, the seam marks, the timing pair and
 * last_kernel_ms --; the call is outside the run's event pair; the plan need not hold velocities.
 *   windowed plans (3e, nz > 238) are supported: only OWNED levels are read, each with lo, hi and the weight of the tall
 *     level it stands for, in rising order of the tall level; k in kbot and ktop is the TALL level; the running values
 *     stay in registers across the windows; no seam refresh is launched.
 *   no output is reached by the phantom half of an odd fp32 plan (3f), the partner of a split fp32 pair, padding slots or
 *     instances outside the block, and no byte outside the outputs is written.
 * A kernel of its own on every kind of plan (mpdata_column_cond.hip), not fused into the run.  Wave-major and windowed
 * plans: the staging of 3k -- a workgroup copies the column slots of a group of adjacent instances and a batch of columns
 * through LDS as linear streams, with the rows wgt, lo and hi of those instances; a lane per (instance element, column)
 * walks its levels from LDS in rising order.  The condition tracer is staged ONCE per workgroup and batch: the lane keeps
 * the in-bits of its levels in registers (eight 32-bit words per half, all at compile-time positions), forms kcnt, kbot
 * and ktop from them with integer bit operations (exact), and the value tracers follow through the same columns of LDS
 * in a loop inside the kernel, each summed under the bits.  (Windowed plans carry the running sums of up to eight value
 * tracers across the windows in registers; a ninth tracer stages the condition a second time.)  With cpath == NULL only
 * tc is staged.  No reduction across lanes; a store of an (n, nx) row of a full group is a whole 128-byte line.
 * Reference-layout plans and the array forms: one thread per (instance, column), coalesced along the instances, the
 * loops over k and the tracers inside, 64-bit offsets.
 * Checked before any device call, in this order -- a failed call changes nothing:
 * MPDATA_EINVAL: null plan, n < 1, a range outside [0, ncrms), tc outside [0, ntracers), lo and hi both NULL, every output
 * NULL, cover without kcnt or mass without cpath, with a non-null cpath a tracer range that is empty or outside the plan;
 * in the array forms bad sizes (ncrms < 1, nx < 1, nz < 2, ntracers < 1), a block outside the arrays, a null f, rho or
 * adz, then the same list as above.
 * MPDATA_EUNSUPPORTED: a multi-GPU handle, as in 3d - 3v (take mpdata_plan_shard_plan(plan, g) and a shard-local sl0).
 * MPDATA_ESTATE: a host form of the other precision; a plan never filled.
 * Time on the MI355X (docs/EXPERIMENTS.md AG, tools/column_cond_bench.py, profiles/column_cond_bench.json), 65536 x 32 x 28,
 * cold, plans of nine tracers, lo and hi given, 40 % of the levels in, fp64 / fp32: kcnt + cover 0.182 / 0.126 ms; cpath of T = 1,
 * 3, 8 value tracers 0.270 / 0.183, 0.462 / 0.306, 0.908 / 0.622 ms -- 3.4 / 2.5, 3.9 / 3.0, 4.5 / 3.3 TB/s of the algorithmic bytes, the
 * interior of the T + 1 tracers read once.  Against existing calls in the same run on the same plans: (a)
 * mpdata_plan_export_device of the T + 1 tracers (the old route without the caller's kernel): 0.87 x / 1.09 x for kcnt + cover,
 * 0.66 x / 0.83 x, 0.58 x / 0.72 x, 0.51 x / 0.66 x for T = 1, 3, 8; (b) mpdata_plan_column_path_device of T + 1 tracers, the same bytes
 * through the same staging: 1.43 x / 1.66 x, 1.09 x / 1.30 x, 0.96 x / 1.13 x, 0.85 x / 1.04 x.  Said plainly: the count alone beats the
 * export by little in fp64 and LOSES to it in fp32; the call loses to column_path until three (fp64) or more than eight (fp32)
 * value tracers share the condition.  Tall plans, 4096 x 32 x 300 (6 windows): 0.539 / 0.388, 0.809 / 0.580, 1.367 / 0.976, 2.771 / 1.962
 * ms -- it LOSES to the export everywhere there (3.2 x / 2.7 x for the count, 1.9 x / 1.6 x at T = 8) and to column_path by 1.5 x to 2.2 x:
 * two columns fit next to the three rows at 55 levels.  A block of 64 instances: 0.020 / 0.029 ms. */
/* instances [sl0, sl0+n) of a resident plan; whole plan: sl0 = 0, n = ncrms.  Device arrays of the plan's precision on
 * the plan's device, asynchronous on the plan's stream. */
int mpdata_plan_column_cond_device(mpdata_plan* plan, int64_t sl0, int64_t n, int tc, const void* lo, const void* hi, void* kcnt,
                                   void* kbot, void* ktop, void* cpath, void* cover, void* mass, int first_tracer, int ntracers);
/* host arrays, all tracers (cpath (n, nx, ntracers of the plan), mass (n, ntracers of the plan)), synchronous (the
 * plan's block staging buffer, as the 3g - 3v host forms) */
int mpdata_plan_column_cond(mpdata_plan* plan, int64_t sl0, int64_t n, int tc, const double* lo, const double* hi, double* kcnt,
                            double* kbot, double* ktop, double* cpath, double* cover, double* mass);
int mpdata_plan_column_cond_f32(mpdata_plan* plan, int64_t sl0, int64_t n, int tc, const float* lo, const float* hi, float* kcnt,
                                float* kbot, float* ktop, float* cpath, float* cover, float* mass);
/* the same on instances [sl0, sl0+n) of reference-layout DEVICE arrays f(ncrms,-2:nx+3,1,nzm,ntracers), rho(ncrms,nzm),
 * adz(ncrms,nzm) (leading dimension ncrms), which are only read; lo, hi and the outputs as above (leading dimension n;
 * cpath (n, nx, ntr), mass (n, ntr)).  Asynchronous on `stream`; 64-bit offsets. */
int mpdata_column_cond_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, const double* f,
                              const double* rho, const double* adz, int tc, const double* lo, const double* hi, double* kcnt,
                              double* kbot, double* ktop, double* cpath, double* cover, double* mass, int first_tracer, int ntr,
                              void* stream);
int mpdata_column_cond_f32_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, const float* f,
                                  const float* rho, const float* adz, int tc, const float* lo, const float* hi, float* kcnt,
                                  float* kbot, float* ktop, float* cpath, float* cover, float* mass, int first_tracer, int ntr,
                                  void* stream);

/* ---- 3x. A conservative per-level non-negativity fixer of a resident plan's tracers, in place (what a SAM-type host
 * model runs after a step that can drive a positive-definite tracer below zero -- 3i and 3p without CLIP, 3m with a
 * Courant number above one, 3t without LIMIT, 3l near its stability limit, 3o with a caller's matrix: the negative cells
 * of a level are set to zero and the level's other cells are scaled so that the level's total is what it was.  The CLIP
 * modes of 3i and 3p clip and create mass; this call does not).  This section is the specification; the reference tree
 * has no such routine.  For instance sl in [sl0, sl0 + n), tracer t in [first_tracer, first_tracer + ntracers), level
 * k = 1 .. nzm, nzm = nz - 1, interior column i = 1 .. nx, with b = sl - sl0:
 *   s = +0;  p = +0;  c = +0
 *   do i = 1, nx:  x = f_old(sl,i,k,t)
 *                  s = s + x                      (the sum of 3g, in its order: the same bits as level_stats)
 *                  y = (x > 0) ? x : +0           (compare-and-select; -0.0 and negatives give +0)
 *                  p = p + y
 *                  c = c + ((x < 0) ? 1 : 0)
 *   sum(b,k,t) = s;  nneg(b,k,t) = c              (each optional; c as a real of the plan's precision, as cnt of 3v)
 *   c == 0       :  f(sl,:,k,t) keeps every bit -- the row is not rewritten; a -0.0 there stays
 *   c > 0, s > 0 :  r = s / p (ONE IEEE divide, correctly rounded in both precisions);  f(sl,i,k,t) = y_i * r
 *   c > 0, else  :  f(sl,i,k,t) = +0 for every i  (the row owes mass; sum tells the caller how much)
 * Every operation is rounded ONCE in the plan's precision, in exactly this association; nothing is contracted, so EXACT
 * and FAST plans give the same bits.  NaN and infinities are outside the contract.  r is whatever the divide gives: it
 * is at most 1 up to rounding, it can be exactly 1 (a negative cell far below the row's unit roundoff), and it is not
 * clamped.  A fixed row sums to s up to (2 nx + 4) u sum|f_old| (two sequential sums, the divide, the products), and a
 * second call finds nneg == 0 everywhere and changes nothing.
 * Both arrays are of the plan's precision, reference layout, instance index fastest, leading dimension n (the block's
 * first instance at index 0), tightly packed, tracer slowest:
 *   sum   (n, nzm [, ntracers])   only written; may be NULL
 *   nneg  (n, nzm [, ntracers])   only written; may be NULL
 * With both NULL the call is still valid.  No byte outside these arrays is read or written.  Afterwards the plan behaves
 * exactly as if the interior of f had been exported, changed as above and imported again.
 * Towards the rest of a plan (3r's rules, word for word):
 *   halo marks   only interior columns are read and written; halo columns are neither.  GIVEN plans: halos keep every
 *     bit.  PERIODIC plans: no wrap is launched, because the sums are taken over the interior alone; the halo marks of
 *     the range are cleared afterwards, so the next run or read-back hands out wrapped halos of the new field.
 *   windowed plans (3e, nz > 238) are supported: the call reads and writes OWNED levels only, needs no seam refresh in
 *     front, and clears the seam marks of the range afterwards.  sum and nneg of a level are written by that level's
 *     owner and are addressed by tall level directly in the caller's arrays: nothing is cut into windows.
 *   odd fp32 plans (3f)  the phantom half follows instance ncrms - 1 whenever the block holds it and its row is
 *     rewritten (on a windowed plan the phantom of the inner plan is restored behind the call, as in 3m / 3n / 3p / 3r).
 *   untouched    an fp32 block that splits a pair stores the partner back as loaded: a -0.0 or a negative value there
 *     stays; padding slots, neighbours in a tile, instances and tracers outside the ranges, flux, u, w, rho, rhow, adz,
 *     the held-velocity flags, the boundary mode and the timing pair keep every bit.  The call is outside the run's
 *     event pair; the plan need not hold velocities.
 * A kernel of its own on every kind of plan (mpdata_nonneg.hip), not fused into the run.  Wave-major and windowed plans: a
 * lane owns one (instance, level) element and walks its interior column slots (the walk of 3g, 3i and 3r), so the three
 * reductions are lane-local: no LDS, no barrier, no cross-lane traffic, and no ordering to argue.  Two forms (DESIGN.md
 * 4.27): nx <= 32, the KEPT form -- the nx columns of the lane's element are loaded into registers once (fully unrolled,
 * no scratch), reduced, and scaled and stored by the lanes whose row is in need; nx > 32, the RE-READ form -- a reducing
 * walk, the outputs, and, unless no lane of the wave is in need, the updating walk over the same columns.  Both give the
 * same bits.  A row without a negative cell is read and never stored: on a field that is already clean the call is a
 * read.  Reference-layout plans and the array forms: one thread per instance and (level, tracer) row, two loops over i,
 * in place, no scratch array.
 * Checked before any device call, in this order -- a failed call changes nothing:
 * MPDATA_EINVAL: null plan, n < 1, a range outside [0, ncrms), a bad tracer range; in the array forms bad sizes
 * (ncrms < 1, nx < 1, nz < 2, ntracers < 1), a block outside the arrays, then a null f.
 * MPDATA_EUNSUPPORTED: a multi-GPU handle, as in 3d - 3w (take mpdata_plan_shard_plan(plan, g) and a shard-local sl0).
 * MPDATA_ESTATE: a host form of the other precision; a plan never filled.
 * Not offered (follow-ups): a floor other than zero; borrowing along the column (a vertical fixer in the staging of 3k);
 * fusing the fixer into 3q.
 * Time on the MI355X (docs/EXPERIMENTS.md AH, tools/nonneg_bench.py, profiles/nonneg_bench.json), 65536 x 32 x 28, one tracer,
 * cold, fp64 / fp32: (a) a field without a negative cell 0.091 / 0.052 ms -- 0.84 x / 0.85 x mpdata_plan_level_stats_device
 * (sum), which reads the same bytes (0.108 / 0.061 ms), 5.0 / 4.4 TB/s of the interior of f read once; (b) every row in need
 * 0.216 / 0.113 ms -- 1.00 x / 1.05 x mpdata_plan_relax_device in mean mode, which moves the same bytes (0.216 / 0.108 ms), 4.2 /
 * 4.0 TB/s of the interior read once and written once; with both outputs 0.236 / 0.121 ms; (c) the mix of the tests (71 % of
 * the rows in need) 0.223 / 0.113 ms.  Against mpdata_plan_export_device + mpdata_plan_import_device of f alone, the old route
 * without the caller's kernel (0.448 / 0.238 ms): (a) 0.20 x / 0.22 x, (b) 0.48 x / 0.47 x, (c) 0.50 x / 0.47 x.  With 25
 * tracers: (a) 2.01 / 1.06 ms, (b) 5.38 / 2.78 ms (0.99 x / 1.02 x relax, 0.51 x / 0.53 x the round trip).  Tall plans, 4096 x 32
 * x 300 (6 windows): (a) 0.065 / 0.036 ms (0.79 x / 0.73 x level_stats), (b) 0.151 / 0.083 ms (1.01 x / 1.09 x relax, 0.40 x /
 * 0.27 x the round trip).  The KEPT form against the RE-READ form at nx = 32 on (b): 0.216 against 0.228 ms fp64, 0.113 / 0.125
 * fp32, 0.151 / 0.170 and 0.083 / 0.094 tall -- 5 % to 12 % (10 % to 18 % on the mix), where five rounds of one form differ by
 * 3 % (tall: 4 %) at most.  Said plainly: (b) does not beat relax -- in fp32 it is 5 % (tall: 9 %) slower, with three running sums per
 * half where relax has one --, and the mix is no faster than (b) although it stores 71 % of the rows: a lane that returns
 * early frees nothing while the other lanes of its wave store. */
/* instances [sl0, sl0+n) of a resident plan; whole plan: sl0 = 0, n = ncrms.  Device arrays of the plan's precision on
 * the plan's device, asynchronous on the plan's stream. */
int mpdata_plan_nonneg_device(mpdata_plan* plan, int64_t sl0, int64_t n, void* sum, void* nneg, int first_tracer, int ntracers);
/* host arrays, all tracers, synchronous (the plan's block staging buffer, as the 3g - 3w host forms) */
int mpdata_plan_nonneg(mpdata_plan* plan, int64_t sl0, int64_t n, double* sum, double* nneg);
int mpdata_plan_nonneg_f32(mpdata_plan* plan, int64_t sl0, int64_t n, float* sum, float* nneg);
/* the same on instances [sl0, sl0+n) of a reference-layout DEVICE array f(ncrms,-2:nx+3,1,nzm[,ntracers]) (leading
 * dimension ncrms); sum, nneg as above (leading dimension n).  Asynchronous on `stream`; 64-bit offsets. */
int mpdata_nonneg_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, double* f, double* sum, double* nneg,
                         void* stream);
int mpdata_nonneg_f32_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, float* f, float* sum, float* nneg,
                             void* stream);

/* ---- 3y. Saturation adjustment of a resident plan's tracers, in place (the one step of a cloud model's scalar loop that
 * still forced an export, a caller's kernel and an import: diagnosing the condensate, and the temperature that goes with
 * it, from a conserved temperature-like tracer and total water -- SAM's `cloud`.  It makes the cloud water that 3t turns
 * into rain and that 3v and 3w count as cloud fraction, base and top).  This section is the specification; the reference
 * tree has no such routine.  All the physics is in the caller's numbers: the library hard-codes no constant.
 * Rounding: every statement below is rounded once in the plan's precision, in this association, with nothing contracted;
 * every `/` is a correctly rounded IEEE division; every comparison is plain compare-and-select, never fmax / fmin, so NaN
 * and -0 take the "else" value.  EXACT and FAST plans give the same bits.
 * Parameters: a host struct, passed by const pointer and read before the call returns.  Every double is rounded once to the
 * plan's precision; three derived values are formed on the host in the plan's precision, each operation rounded once:
 *   an = 1 / (tmax - tmin);   bn = tmin * an;   lf = ls - lv
 * Scope: four distinct tracers -- th (input, the temperature-like tracer), tq (input, total water), tn (output, the
 * condensate: overwritten), tt (optional output, the temperature; -1: absent) --, every instance sl in [sl0, sl0 + n) with
 * b = sl - sl0, every level k = 1 .. nzm, nzm = nz - 1, and every INTERIOR column i = 1 .. nx.
 * Rows: pres (required, in the unit of es) and gz (optional, NULL: T1 = h) are (n, nzm) arrays of the plan's precision,
 * reference layout, instance index fastest, leading dimension n (the block's first instance at index 0), as r of 3t.
 * p = pres(b,k), and rp = 1 / p is formed once per row.  Per cell:
 *   pres(b,k) == 0 : the row keeps every bit of tn and tt and is not stored; ncld(b,k) = iters(b,k) = +0
 *   h = f(i,k,th);  q = f(i,k,tq);  qq = (q > 0) ? q : +0;   T1 = gz ? h - gz(b,k) : h
 *   curve(c, dc, T):  x = T - t0;  x = (x > xmin) ? x : xmin
 *                     es = c[8]; for j = 7..0: es = c[j] + x * es          (de likewise from dc)
 *                     pm = p - es;  den = (pm > es) ? pm : es;  qs = (eps * es) / den;  dq = (eps * de) * rp
 *   sat(T):  without ICE, or T >= tmax :  (qs, dq) = curve(esw, desw, T);  L = lv;  dL = +0
 *            ICE and T <= tmin         :  (qs, dq) = curve(esi, desi, T);  L = ls;  dL = +0
 *            else: om = an * T - bn;  u = 1 - om;  (qw, dw), (qi, di) from the two curves;
 *                  qs = om * qw + u * qi;  dq = om * dw + u * di;  L = lv + u * lf;  dL = an * lf
 *   (qs, ..) = sat(T1);  T = T1
 *   qq > qs :  it = 0
 *              repeat: (qs, dq, L, dL) = sat(T);  e = qq - qs
 *                      fff = (T1 - T) + L * e;  dfff = (dL * e - L * dq) - 1;  d = -fff / dfff
 *                      T = T + d;  it = it + 1
 *              while |d| > tol and it < maxit
 *              qs = qs + dq * d;  qn = qq - qs;  qn = (qn > 0) ? qn : +0
 *   else    :  qn = +0;  it = 0
 *   f(i,k,tn) = qn;   tt >= 0 : f(i,k,tt) = T
 *   ncld(b,k)  = number of interior columns with qn > 0       (optional output, NULL: skipped)
 *   iters(b,k) = maximum of it over the interior columns      (optional output, NULL: skipped)
 * ncld and iters are (n, nzm) reals of the plan's precision, like cnt of 3v.  th and tq are only read and keep every bit.
 * Halo columns are neither read nor written.  Every tracer other than tn and tt keeps every bit.  The regime branches are
 * selects by definition, so a wave may skip a curve that none of its lanes needs without changing a bit.  A cell stops
 * iterating on ITS OWN d, whatever its neighbours in the wave do.  Without ICE esi, desi, ls, tmin and tmax reach no result.
 * Towards the rest of a plan, as in 3t, for the written tracers tn and tt:
 *   halo marks   PERIODIC plans: no wrap is launched; the halo marks of tn and tt are cleared afterwards.
 *   windowed plans (3e, nz > 238) are supported: owned levels only, each with pres and gz of the tall level it stands for;
 *     no seam refresh in front; the seam marks of tn and tt are cleared afterwards.
 *   odd fp32 plans (3f)  the phantom half follows instance ncrms - 1 in tn and tt wherever the block holds it and its pres
 *     is not zero (on a windowed plan the host restores the inner plan's phantom behind the call, as in 3t).
 *   untouched    the partner of a split fp32 pair, padding slots and instances outside the block keep every bit; the marks
 *     of th and tq do not change.  The plan need not hold velocities; the call is outside the run's event pair.
 * A kernel of its own on every kind of plan (mpdata_satadj.hip).  Wave-major and windowed plans: the lane-owned walk of 3t;
 * p, rp and gz in registers per half; two read streams and one or two write streams at signed 64-bit tracer offsets; no
 * LDS, no barrier, no cross-lane traffic but the __ballot that decides whether a wave goes on iterating (and whether it
 * needs a curve).  The Newton loop is predicated per lane and per half -- a finished cell keeps its T, qs, dq, d by select
 * -- and the loops of several columns of a lane run interleaved under one joint exit, so that their dependent Horner chains
 * overlap.  Templates on ICE and on tt: the warm-only kernel carries neither the second curve nor the second store stream.
 * Reference-layout plans and the array forms: one thread per instance and level row, one loop over i.
 * Checked before any device call, in this order -- a failed call changes nothing:
 * MPDATA_EINVAL: null plan; n < 1 or a block outside [0, ncrms); th, tq or tn outside [0, ntracers); tt outside
 * [-1, ntracers); any two of the given tracers equal; null pres; null par; maxit outside 1 .. 32; tol not >= 0; with ICE,
 * tmax not > tmin; a mode bit other than MPDATA_SATADJ_ICE; in the array forms the size, block and null-f checks of 3t first.
 * MPDATA_EUNSUPPORTED: a multi-GPU handle, as in 3d - 3x.  MPDATA_ESTATE: a host form of the other precision; a plan never
 * filled.
 * Time on the MI355X (docs/EXPERIMENTS.md AI, tools/satadj_bench.py, profiles/satadj_bench.json), 65536 x 32 x 28, four tracers,
 * cold, ICE and tt, fp64 / fp32: no cell saturated 0.466 / 0.277 ms; the recipe's mix (37.5 % of the cells saturated, 1 to 6
 * steps) 1.906 / 1.313 ms; the mix sorted so that saturated cells fill whole rows and waves 0.970 / 0.614 ms.  Warm only, no tt:
 * 0.340 / 0.179, 1.133 / 0.727, 0.608 / 0.349 ms.  Against existing calls in the same run: (a) export_device of th, tq +
 * import_device of tn, tt, the old route without the caller's kernel (0.851 / 0.423 ms): 0.55 x / 0.65 x dry, 2.24 x / 3.10 x on the
 * mix, 1.14 x / 1.45 x sorted; (b) mpdata_plan_convert_device with every option, the same two reads and two writes (0.422 /
 * 0.221 ms): 1.11 x / 1.25 x dry, 4.52 x / 5.94 x on the mix -- the call is bound by the vector unit, not by bytes, wherever cells
 * are saturated; (c) mix over sorted 1.97 x / 2.14 x: divergence inside a wave doubles the time; (d) columns interleaved per lane
 * (MPDATA_SATADJ_NC), mix: 1: 1.915 / 1.247 ms, 2: 1.902 / 1.306, 4: 2.001 / 1.634, 8: 3.393 / 2.668 -- interleaving does not pay (it
 * costs registers, hence waves per SIMD, and the waves overlap the chains as well); 2 is kept, level with 1 in fp64 and 4.5 %
 * behind it in fp32.  A block of 64 instances: 0.137 / 0.185 ms.  4096 x 32 x 300 (6 windows): dry 0.433 / 0.235 ms, mix 1.133 / 0.848
 * ms, 1.50 x / 1.40 x (a).  Said plainly: on the mix the call LOSES to the bare export + import; what it saves is the caller's own
 * kernel on top of that route, the staging memory and two passes over f. */
typedef struct mpdata_satadj_params {
  double esw[9], desw[9]; /* liquid: es(x), d es / dT (x) as degree-8 polynomials in x, Horner from [8] down */
  double esi[9], desi[9]; /* ice: the same; read only with MPDATA_SATADJ_ICE */
  double t0, xmin;        /* x = T - t0;  x = (x > xmin) ? x : xmin */
  double eps;             /* qs = (eps * es) / max(es, p - es) */
  double lv, ls;          /* L / cp of condensation and of sublimation, in the unit of the temperature tracer */
  double tmin, tmax;      /* the mixed-phase ramp, tmin < tmax; ICE only */
  double tol;             /* Newton stops when |dT| <= tol ... */
  int maxit;              /* ... or after maxit steps, 1 <= maxit <= 32 */
} mpdata_satadj_params;
#define MPDATA_SATADJ_ICE 1 /* mode bit: the ice curve below tmin and the linear ramp between tmin and tmax */
/* instances [sl0, sl0+n) of a resident plan; whole plan: sl0 = 0, n = ncrms.  Device arrays of the plan's precision on
 * the plan's device, asynchronous on the plan's stream. */
int mpdata_plan_satadj_device(mpdata_plan* plan, int64_t sl0, int64_t n, int th, int tq, int tn, int tt, const void* pres,
                              const void* gz, const mpdata_satadj_params* par, int mode, void* ncld, void* iters);
/* host arrays, synchronous (the plan's block staging buffer, as the 3g - 3x host forms) */
int mpdata_plan_satadj(mpdata_plan* plan, int64_t sl0, int64_t n, int th, int tq, int tn, int tt, const double* pres,
                       const double* gz, const mpdata_satadj_params* par, int mode, double* ncld, double* iters);
int mpdata_plan_satadj_f32(mpdata_plan* plan, int64_t sl0, int64_t n, int th, int tq, int tn, int tt, const float* pres,
                           const float* gz, const mpdata_satadj_params* par, int mode, float* ncld, float* iters);
/* the same on instances [sl0, sl0+n) of a reference-layout DEVICE array f(ncrms,-2:nx+3,1,nzm,ntracers) (leading
 * dimension ncrms); pres, gz, ncld, iters as above (leading dimension n).  Asynchronous on `stream`; 64-bit offsets. */
int mpdata_satadj_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, double* f, int th, int tq, int tn,
                         int tt, const double* pres, const double* gz, const mpdata_satadj_params* par, int mode, double* ncld,
                         double* iters, void* stream);
int mpdata_satadj_f32_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, float* f, int th, int tq, int tn,
                             int tt, const float* pres, const float* gz, const mpdata_satadj_params* par, int mode, float* ncld,
                             float* iters, void* stream);

/* ---- 3z. Linear combinations of a resident plan's tracers, in place (what is left of a cloud model's scalar loop once 3t and
 * 3y hold its microphysical state: the fields DERIVED from that state -- the buoyancy, a level-dependent linear combination
 * of temperature, vapour, cloud and precipitating water plus a level constant; total water qt = qv + qn in front of 3y and
 * qv = qt - qn behind it; liquid/ice static energy from T and the condensates; a snapshot of a tracer in front of a step and
 * the tendency (f_new - f_old) / dt behind it; a tracer set to a profile; any a * x + b * y between tracers.  3t couples
 * exactly two tracers by one fixed formula and every other call of 3g - 3y sees one tracer at a time; this one builds one
 * tracer from a list).  This section is the specification; the reference tree has no such routine.  For one destination
 * tracer dst and a list of nsrc source tracers src[0 .. nsrc-1] (a host array of int, read during the call), every instance
 * sl in [sl0, sl0 + n) with b = sl - sl0, every level k = 1 .. nzm, nzm = nz - 1, and every INTERIOR column i = 1 .. nx, with
 * x_j = f_old(i,k,src[j]) -- the OLD value also where src[j] == dst --, every statement below is rounded once in the plan's
 * precision, in this association, with no contraction; comparisons are plain compare-and-select, never fmax / fmin:
 *   nsrc >= 1:  v = coef ? coef(b,k,0) * x_0 : x_0
 *               do j = 1, nsrc-1:  p = coef ? coef(b,k,j) * x_j : x_j ;  v = v + p
 *               c0 given:  v = v + c0(b,k)
 *   nsrc == 0:  v = c0(b,k)                                (c0 required)
 *   mode & MPDATA_COMBINE_CLIP:  v = (v > 0) ? v : +0      (so NaN and -0 give +0)
 *   f(i,k,dst) = v
 *   sum(b,k):  s = +0; do i = 1, nx: s = s + v(i)          (NULL: skipped; the sum of 3g of the NEW dst row)
 * coef (optional input, (n, nzm, nsrc), coef(b,k,j) at b + n * (k + nzm * j); NULL: no multiply at all -- with nsrc == 1 and
 * no c0 the call is then a bit copy: every NaN payload and every -0.0 is preserved), c0 (optional input, (n, nzm)) and sum
 * (optional output, (n, nzm)) are arrays of the plan's precision, reference layout, instance index fastest, leading
 * dimension n (the block's first instance at index 0), as r of 3t.  nsrc lies in [0, MPDATA_COMBINE_MAX]; sources may
 * repeat; dst may be among the sources (the in-place form, f_dst = 2 f_dst - f_t): all loads of a cell precede its store.
 * Halo columns are neither read nor written.  A tracer other than dst keeps every bit.  EXACT and FAST plans give the same
 * bits.  No byte outside the arrays is read or written.  Afterwards the plan behaves exactly as if the interior of dst had
 * been exported, set as above and imported again.
 * Towards the rest of a plan, for the one written tracer dst:
 *   halo marks   only interior columns are read and written.  GIVEN plans: halos keep every bit.  PERIODIC plans: no wrap
 *     is launched; the halo mark of dst is cleared afterwards, so the next run or read-back hands out wrapped halos of the
 *     new field.  The sources' marks are not touched.
 *   windowed plans (3e, nz > 238) are supported, as in 3t: the operator is pointwise, the call reads and writes OWNED levels
 *     only, each with coef and c0 of the tall level it stands for, needs no seam refresh in front and clears the seam mark
 *     of dst afterwards; sum of a level is written by that level's owner.
 *   odd fp32 plans (3f)  the phantom half follows instance ncrms - 1 in dst whenever the block holds it (on a windowed plan
 *     the phantom of the inner plan is restored behind the call, as in 3t).
 *   untouched    an fp32 block that splits a pair stores the partner back as loaded: a -0.0 there stays; padding slots,
 *     neighbours in a tile, instances outside the block, every other tracer, flux, u, w, rho, rhow, adz, the held-velocity
 *     flags, the boundary mode and the timing pair keep every bit.  The call is outside the run's event pair; the plan need
 *     not hold velocities.
 * A kernel of its own on every kind of plan (mpdata_combine.hip), not fused into the run.  Wave-major and windowed plans: the
 * lane-owned walk of 3t with 1 + nsrc streams: the dst tracer is the base and every source lies at a signed 64-bit offset from
 * it; the kernel is a template on nsrc, with 8 columns in flight per source for 0 to 2 sources, 4 for 3 and 4, and for 5
 * to 8 sources 3 on fp64 and 2 on fp32 plans (8 to 24 loads in flight per lane; no kernel above 128 VGPRs, none with scratch).  coef and c0 are in registers, sum is
 * lane-local in column order: no LDS, no barrier, no cross-lane traffic.  nsrc == 0 loads nothing from f; a wave none of whose
 * elements lies in the block loads and stores nothing.  Reference-layout plans and the array forms: one thread per instance
 * and level row, one loop over i, in place.
 * Checked before any device call, in this order -- a failed call changes nothing:
 * MPDATA_EINVAL: null plan; n < 1 or a range outside [0, ncrms); dst outside [0, ntracers); nsrc outside
 * [0, MPDATA_COMBINE_MAX]; nsrc > 0 with a null src; a src[j] outside [0, ntracers); nsrc == 0 with a null c0; a mode bit other
 * than MPDATA_COMBINE_CLIP; in the array forms bad sizes (ncrms < 1, nx < 1, nz < 2, ntracers < 1), a block outside the arrays,
 * a null f, then dst, nsrc, src, c0 and the mode as above.
 * MPDATA_EUNSUPPORTED: a multi-GPU handle, as in 3d - 3y (take mpdata_plan_shard_plan(plan, g) and a shard-local sl0).
 * MPDATA_ESTATE: a host form of the other precision; a plan never filled.
 * Time on the MI355X (docs/EXPERIMENTS.md AJ, tools/combine_bench.py, profiles/combine_bench.json), 65536 x 32 x 28, nine tracers,
 * cold, nsrc = 0 / 1 / 2 / 4 / 8 distinct sources with coef, c0 and sum: 0.121 / 0.214 / 0.307 / 0.507 / 0.894 ms fp64, 0.054 / 0.109 /
 * 0.152 / 0.261 / 0.474 ms fp32 -- 3.7 / 4.2 / 4.4 / 4.5 / 4.6 TB/s fp64 of the algorithmic bytes (the interior of nsrc tracers read and
 * one written); without coef, c0 and sum 1 % to 10 % less (the copy: 0.203 / 0.099 ms).  Against existing calls in the same run:
 * (a) 0.60 x / 0.51 x / 0.50 x / 0.49 x / 0.48 x fp64 and 0.50 x to 0.46 x fp32 mpdata_plan_export_device of the nsrc sources +
 * mpdata_plan_import_device of dst (the old route without the caller's kernel); (b) nsrc = 1: 0.97 x fp64, 0.90 x fp32 one
 * mpdata_plan_level_add_device; (c) nsrc = 2: 0.75 x mpdata_plan_convert_device with r alone, which writes one tracer more.  The
 * in-place form costs 3 % to 6 % more.  A block of 64 instances, 8 sources: 0.013 / 0.019 ms.  Tall plans, 4096 x 32 x 300 (6
 * windows): 0.107 / 0.187 / 0.255 / 0.396 / 0.659 ms fp64, 0.079 / 0.107 / 0.142 / 0.220 / 0.380 ms fp32, 0.54 x to 0.44 x and 0.49 x to
 * 0.29 x (a).  Said plainly: on tall plans one source LOSES to level_add (1.23 x fp64, 1.27 x fp32), and the write-only form
 * nsrc = 0 is the slowest per byte (2.0 to 2.9 TB/s there).  Columns in flight, timed per class on libraries of their own: 8 / 4
 * are the fastest or within 1 % for 0 to 4 sources; for 5 to 8 sources 3 beat 2 by 3.9 % in fp64 and lose by 1.5 % in fp32, which
 * is what is kept -- differences that two processes of one session do not resolve (identical kernels differ by up to 3 %). */
#define MPDATA_COMBINE_CLIP 1 /* mode bit: v = (v > 0) ? v : +0 in front of the store */
#define MPDATA_COMBINE_MAX 8  /* the sources of one call at most */
/* instances [sl0, sl0+n) of a resident plan; whole plan: sl0 = 0, n = ncrms.  src: a HOST array of nsrc ints in every form.
 * Device arrays of the plan's precision on the plan's device, asynchronous on the plan's stream. */
int mpdata_plan_combine_device(mpdata_plan* plan, int64_t sl0, int64_t n, int dst, int nsrc, const int* src, const void* coef,
                               const void* c0, int mode, void* sum);
/* host arrays, synchronous (the plan's block staging buffer, as the 3g - 3y host forms) */
int mpdata_plan_combine(mpdata_plan* plan, int64_t sl0, int64_t n, int dst, int nsrc, const int* src, const double* coef,
                        const double* c0, int mode, double* sum);
int mpdata_plan_combine_f32(mpdata_plan* plan, int64_t sl0, int64_t n, int dst, int nsrc, const int* src, const float* coef,
                            const float* c0, int mode, float* sum);
/* the same on instances [sl0, sl0+n) of a reference-layout DEVICE array f(ncrms,-2:nx+3,1,nzm,ntracers) (leading
 * dimension ncrms); coef, c0, sum as above (leading dimension n).  Asynchronous on `stream`; 64-bit offsets. */
int mpdata_combine_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, double* f, int dst, int nsrc,
                          const int* src, const double* coef, const double* c0, int mode, double* sum, void* stream);
int mpdata_combine_f32_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, float* f, int dst, int nsrc,
                              const int* src, const float* coef, const float* c0, int mode, float* sum, void* stream);

/* ---- 3aa. Running column integrals of a resident plan's tracers, in place (the calls along the levels of 3g - 3z either
 * reduce a column to one number, 3k and 3w, or solve a recurrence in it, 3o, 3q and 3s; none hands out the RUNNING integral,
 * the value at every level of the sum from the surface up to it or from the model top down to it: the water above each level
 * that a radiation or overlap scheme reads, the hydrostatic pressure perturbation that belongs to the buoyancy 3z builds,
 * integrated downward, the cumulative flux of a column of sources or sinks, which 3n offers for its own wp * f only).  This
 * section is the specification; the reference tree has no such routine.  For a source tracer src and a destination tracer
 * dst, every instance sl in [sl0, sl0 + n) with b = sl - sl0 and every INTERIOR column i = 1 .. nx, with nzm = nz - 1,
 * everything in the plan's precision, every statement below one rounded operation, with no contraction, every f the value
 * before the call:
 *   p(k) = wgt(b,k) * f(sl,i,k,src)                       the product rounded; no fma
 *   UP (default):  s = +0.0;  k = 1 .. nzm
 *   DOWN:          s = +0.0;  k = nzm .. 1
 *      inclusive (default):  s = s + p(k);  o(k) = s
 *      EXCLUSIVE:            o(k) = s;      s = s + p(k)
 *   f(sl,i,k,dst) = o(k);     total(b,i) = the final s
 * mode is an OR of MPDATA_COLUMN_SCAN_DOWN and MPDATA_COLUMN_SCAN_EXCLUSIVE.  wgt (optional input, (n, nzm), wgt(b,k) at
 * b + n * (k - 1)) and total (optional output, (n, nx), total(b,i) at b + n * (i - 1)) are arrays of the plan's precision,
 * reference layout, instance index fastest, leading dimension n (the block's first instance at index 0); on a windowed plan
 * wgt is addressed by the TALL level.  wgt NULL: the weight is rho(sl,k) * adz(sl,k), one rounded multiply, exactly as 3k
 * forms it (on a windowed plan each window uses its own rho and adz); total then has, with UP and in either inclusion
 * mode, the bits of 3k's path.  total NULL: skipped.  dst == src is allowed and means in place.  With dst != src the source
 * keeps every bit, and so does every other tracer.  The first o of an EXCLUSIVE scan is +0.0.  EXACT and FAST plans give the
 * same bits.  NaN and infinities are outside the contract, as in 3k.  No byte outside the arrays is read or written.
 * Afterwards the plan behaves exactly as if the interior of src had been exported, scanned as above and imported into dst.
 * Towards the rest of a plan, for the one written tracer dst:
 *   halo marks   only interior columns of dst are written, and halo columns are never read.  GIVEN plans: dst's halos keep
 *     every bit.  PERIODIC plans: no wrap is launched in front; only the halo mark of dst is cleared afterwards, so the next
 *     run or read-back hands out wrapped halos of the new field.  The mark of src is not touched.
 *   windowed plans (3e, nz > 238 with tall columns on) are supported: the call reads and writes OWNED levels only, which
 *     are right whatever the seams hold, so there is no seam refresh in front; only the seam mark of dst is cleared
 *     afterwards.  UP walks the windows upward and DOWN walks them downward, the running s carried in registers: the merged
 *     result is the tall scan bit for bit, and f is read once and written once on every kind of plan.
 *   odd fp32 plans (3f)  the phantom half follows instance ncrms - 1 in dst whenever the block holds it (on a windowed plan
 *     the phantom of the inner plan is restored behind the call, as in 3m - 3o).
 *   untouched    an fp32 block that splits a pair stores the partner's half of dst back as loaded: a -0.0 there stays;
 *     padding slots, neighbours in a tile, instances outside the block, every other tracer, flux, u, w, rho, rhow, adz, the
 *     held-velocity flags, the boundary mode and the timing pair keep every bit.  The call is outside the run's event pair;
 *     the plan need not hold velocities.
 * A kernel of its own on every kind of plan (mpdata_column_scan.hip), not fused into the run.  Wave-major and windowed
 * plans: the staging of 3k and 3o.  A workgroup copies the column slots of 16 adjacent 8-byte instance elements (fewer where
 * the levels would not fit the 40 KiB of LDS those kernels keep) and a batch of columns of src through LDS as linear
 * streams, the weight row with them; a lane per (instance element, column) sweeps its column in LDS in place, sequential
 * in k, and stores total; the waves store LDS to dst's slots, at a signed 64-bit offset from src's, as the same linear
 * streams.  Every global load of a batch precedes a barrier and every global store follows the sweep's barrier; workgroups
 * own disjoint elements.  Direction and inclusion are uniform values of the launch: one copy of the staging
 * code.  No reduction or scan across lanes.  Reference-layout plans and the array forms: one thread per instance and column
 * owns its column, 64-bit offsets.
 * Checked before any device call, in this order -- a failed call changes nothing:
 * MPDATA_EINVAL: null plan; n < 1 or a range outside [0, ncrms); src, then dst outside [0, ntracers); a mode bit other than
 * the two above; in the array forms bad sizes (ncrms < 1, nx < 1, nz < 2, ntracers < 1), a block outside the arrays, a null
 * f, then a null wgt, then src, dst and the mode as above.
 * MPDATA_EUNSUPPORTED: a multi-GPU handle, as in 3d - 3z (take mpdata_plan_shard_plan(plan, g) and a shard-local sl0).
 * MPDATA_ESTATE: a host form of the other precision; a plan never filled.
 * Time on the MI355X (docs/EXPERIMENTS.md AK, tools/column_scan_bench.py, profiles/column_scan_bench.json): 65536 x 32 x 28,
 * three tracers, cold, tracer 0 into tracer 1 with wgt and total, the median of five rounds: 0.215 ms fp64, 0.115 ms fp32 in
 * each of the four modes -- 4.2 / 3.9 TB/s of the algorithmic bytes (the interior of one tracer read and one written); in
 * place 0.226 / 0.112 ms; without wgt and total the same (0.216 / 0.115 ms).  Against existing calls in the same run on the same
 * plans: (a) 0.81 x fp64, 0.70 x fp32 mpdata_plan_vsolve_device (the same staging, two sweeps, a factor kernel); (b) 1.57 x /
 * 1.55 x mpdata_plan_column_path_device of one tracer (the same staging, read only: the price of the stores); (c) 0.89 x /
 * 0.95 x one mpdata_plan_level_add_device (the same bytes and the halo columns on top, no staging; in fp32 level_add's own
 * rounds spread by 6 %, so that ratio is unresolved); (d) 0.49 x / 0.51 x mpdata_plan_export_device +
 * mpdata_plan_import_device of the tracer (the old route without the caller's kernel).  Tall plans, 4096 x 32 x 300 (6
 * windows): 0.244 / 0.156 ms (2.6 / 2.0 TB/s), in place 0.220 / 0.134 ms; 0.24 x / 0.23 x vsolve, 1.00 x / 0.78 x column_path,
 * 0.62 x / 0.49 x (d).  Said plainly: on tall plans the call LOSES to level_add (1.44 x fp64, 1.72 x fp32).  DOWN against UP:
 * 0.998, 0.998 and 1.001 (plain fp64, plain fp32, tall fp64), below the 0.3 % to 1.1 % by which five rounds spread: unresolved;
 * tall fp32 1.010 at a spread of 0.2 %: DOWN costs 1 % more there, resolved. */
#define MPDATA_COLUMN_SCAN_DOWN 1      /* mode bit: from the model top down, k = nzm .. 1 */
#define MPDATA_COLUMN_SCAN_EXCLUSIVE 2 /* mode bit: o(k) is the sum in front of level k */
/* instances [sl0, sl0+n) of a resident plan; whole plan: sl0 = 0, n = ncrms.  Device arrays of the plan's precision on the
 * plan's device, asynchronous on the plan's stream. */
int mpdata_plan_column_scan_device(mpdata_plan* plan, int64_t sl0, int64_t n, int src, int dst, const void* wgt, void* total,
                                   int mode);
/* host arrays, synchronous (the plan's block staging buffer, as the 3g - 3z host forms) */
int mpdata_plan_column_scan(mpdata_plan* plan, int64_t sl0, int64_t n, int src, int dst, const double* wgt, double* total,
                            int mode);
int mpdata_plan_column_scan_f32(mpdata_plan* plan, int64_t sl0, int64_t n, int src, int dst, const float* wgt, float* total,
                                int mode);
/* the same on instances [sl0, sl0+n) of a reference-layout DEVICE array f(ncrms,-2:nx+3,1,nzm,ntracers) (leading
 * dimension ncrms); wgt (required) and total as above (leading dimension n).  Asynchronous on `stream`; 64-bit offsets. */
int mpdata_column_scan_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, double* f, int src, int dst,
                              const double* wgt, double* total, int mode, void* stream);
int mpdata_column_scan_f32_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, float* f, int src, int dst,
                                  const float* wgt, float* total, int mode, void* stream);

/* ---- 3ab. Per-level histograms of a resident plan's tracers (the fourth kind of horizontal statistic a host model takes
 * from its CRM instances, next to the first moments of 3g, the second moments of 3u and the conditional sums of 3v: the
 * DISTRIBUTION -- the PDF of a tracer per level, a CFAD, mass or tracer content binned by a conserved variable.  3v names
 * the route "a histogram of a tracer per level taken bin by bin": one mpdata_plan_level_cond_device call per bin, each of
 * which reads the condition tracer, and with sums every value tracer, again.  This call bins every column ONCE in one
 * walk over the field).  This section is the specification; the reference tree has no such routine.  For one binned tracer
 * tc, nb bins with 1 <= nb <= MPDATA_LEVEL_HIST_MAX_BINS, a HOST array edges of nb + 1 doubles, a range of value tracers
 * [first_tracer, first_tracer + ntracers) -- tc may lie inside it --, every instance sl in [sl0, sl0 + n) with b = sl - sl0,
 * every level k = 1 .. nzm, nzm = nz - 1, over the INTERIOR columns i = 1 .. nx, with c_i = f(sl,i,k,tc) and v_i =
 * f(sl,i,k,t), every statement below is rounded ONCE in the plan's precision, in this association, with nothing contracted,
 * and the comparisons are plain compare-and-select, so EXACT and FAST plans give the same bits:
 *   e_j = edges[j] rounded once to the plan's precision          j = 0 .. nb
 *   m_i = the number of j in 0 .. nb with c_i > e_j              (0 .. nb + 1)
 *   column i is in bin j = m_i - 1 when 1 <= m_i <= nb, else in no bin
 *   cnt(b,k,j)    :  q = +0;  do i = 1, nx:  if column i in bin j:  q = q + 1
 *   bsum(b,k,j,r) :  s = +0;  do i = 1, nx:  if column i in bin j:  s = s + v_i     (r = t - first_tracer)
 * With the non-decreasing edges the call demands, bin j is the half-open interval (e_j, e_{j+1}] -- the interval of 3v, so
 * cnt(:,:,j) and bsum(:,:,j,:) have the bits of 3v's cnt and csum called with lo = e_j and hi = e_{j+1}.  A column with c_i
 * <= e_0 or c_i > e_nb is in no bin; outer edges of -inf / +inf collect everything.  Equal neighbouring edges make an empty
 * bin.  A NaN in c_i is INSIDE the contract: every comparison is false, m_i = 0, the column is in no bin.  Selection means
 * selection, as in 3v: an excluded v_i never reaches a sum, whatever its bits -- no multiplication by a mask; adding a
 * selected +0 is allowed by 3v's argument.  cnt is a real of the plan's precision and exact (nx < 2^24): an implementation
 * may count in integers and convert.
 * edges is a HOST pointer in EVERY form, the device forms included (as mpdata_satadj_params of 3y): it is read before the
 * call returns and may be reused at once; the edges travel to the kernel as launch arguments.  cnt is (n, nzm, nb), bsum is
 * (n, nzm, nb, ntracers), both of the plan's precision, reference layout, instance index fastest, leading dimension n (the
 * block's first instance at index 0).  Either output may be NULL, not both; with bsum == NULL the tracer range is not
 * looked at.  Sums are SUMS and cnt is a count: the caller divides.
 * Towards the rest of a plan, exactly as 3v: halo columns are never read, so a PERIODIC plan needs no wrap; nothing of the
 * plan's state changes -- filled, have_u, have_w, the halo marks, the seam marks, the timing pair and last_kernel_ms --;
 * the call is outside the run's event pair; the plan need not hold velocities.
 *   windowed plans (3e, nz > 238) are supported: only OWNED levels are read, each is written to the tall level it stands
 *     for, and no seam refresh is launched in front.
 *   no output is reached by the phantom half of an odd fp32 plan (3f), the partner of a split fp32 pair or a padding slot,
 *     and no byte outside cnt and bsum is touched.
 * A kernel of its own on every kind of plan (mpdata_level_hist.hip), not fused into the run.  Wave-major and windowed plans:
 * the lane-owned walk of 3v -- a lane owns one (instance, level) element, for fp32 both halves, and walks its interior
 * column slots as read-only linear streams, 8 columns in flight; the value tracers lie at signed 64-bit offsets from the tc
 * stream and are a loop inside the kernel; every accumulator is lane-local in column order.  The bins of a lane are
 * REGISTERS: a compile-time array of the bin class (4, 8 or 16 bins, the least class that holds the bins of the walk), m_i by
 * one compare per edge of the class (edges behind nb are +inf), then an unrolled chain of selects, s[j] = (m == j + 1) ? s[j]
 * + v : s[j]; no array is indexed at run time.  A walk carries at most 16 bins in fp64 and 8 in fp32 -- wider classes spill
 * scalar registers --, and a call of more bins is one launch per GROUP of bins, each reading tc again.  The counters are 32-bit integers, made reals at the store.  One walk per value
 * tracer over the tc stream and the t stream (one stream for t == tc), the first of which also counts; there is no cache of
 * the bin index per column, tc is read and binned again with every value tracer.  No LDS, no barrier, no cross-lane
 * traffic.  A candidate with lane-private bins in LDS was built outside the tree, timed and not taken: DESIGN.md 4.31 with
 * the timings.  Reference-layout plans and the array forms:
 * one thread per instance and level row, loops over i, 64-bit offsets, groups of 8 bins.
 * Checked before any device call, in this order -- a failed call changes nothing:
 * MPDATA_EINVAL: null plan, n < 1, a range outside [0, ncrms), tc outside [0, ntracers), nb outside [1, 32], null edges, a
 * NaN edge or edges[j] > edges[j+1] (checked on the doubles as given: rounding is monotone), cnt and bsum both NULL, with a
 * non-null bsum a tracer range that is empty or outside the plan; in the array forms bad sizes (ncrms < 1, nx < 1, nz < 2,
 * ntracers < 1), a block outside the arrays, a null f, then the same list as above.
 * MPDATA_EUNSUPPORTED: a multi-GPU handle, as in 3d - 3aa (take mpdata_plan_shard_plan(plan, g) and a shard-local sl0).
 * MPDATA_ESTATE: a host form of the other precision; a plan never filled.
 * Time on the MI355X (docs/EXPERIMENTS.md AL, tools/level_hist_bench.py, profiles/level_hist_bench.json), 65536 x 32 x 28,
 * cold, plans of four tracers, the median of five rounds (their spread at most 1.9 %), fp64 / fp32: cnt alone at nb = 2, 4, 8, 16, 32
 * 0.114 / 0.066, 0.128 / 0.079, 0.176 / 0.115, 0.255 / 0.229, 0.525 / 0.456 ms; cnt and bsum of one value tracer at nb = 8 and 32
 * 0.380 / 0.228 and 1.155 / 0.926 ms, of three 0.771 / 0.515 and 2.570 / 2.070 ms.  Against (a) nb mpdata_plan_level_cond_device
 * calls, the route this replaces: 0.55 x / 0.59 x at nb = 2, 0.31 x / 0.37 x, 0.21 x / 0.28 x, 0.15 x / 0.28 x, 0.16 x / 0.28 x at 4, 8, 16,
 * 32; with sums 0.18 x to 0.29 x.  Against (b) ONE such call, the floor of one read of the same bytes: 1.10 x / 1.09 x at nb = 2,
 * 5.0 x / 7.5 x at nb = 32.  Against (c) mpdata_plan_export_device of the tracers: 0.55 x / 0.58 x at nb = 2, 0.84 x / 1.01 x
 * (unresolved) at 8, 1.22 x / 2.0 x at 16, 2.5 x / 4.0 x at 32.  Said plainly: the call is bound by the vector ALU (about 3 nb
 * operations per cell; 0.85 TB/s at nb = 32) and it LOSES to the export from nb = 16 on in both precisions.  4096 x 32 x 300 (6 windows): cnt 0.093 to 0.618 / 0.062 to 0.651 ms for nb = 2 to 32. */
#define MPDATA_LEVEL_HIST_MAX_BINS 32
/* instances [sl0, sl0+n) of a resident plan; whole plan: sl0 = 0, n = ncrms.  edges: HOST; cnt, bsum: device arrays of the
 * plan's precision on the plan's device, asynchronous on the plan's stream. */
int mpdata_plan_level_hist_device(mpdata_plan* plan, int64_t sl0, int64_t n, int tc, int nb, const double* edges, void* cnt,
                                  void* bsum, int first_tracer, int ntracers);
/* host arrays, all tracers (bsum (n, nzm, nb, ntracers of the plan)), synchronous (the plan's block staging buffer, as the
 * 3g - 3aa host forms) */
int mpdata_plan_level_hist(mpdata_plan* plan, int64_t sl0, int64_t n, int tc, int nb, const double* edges, double* cnt,
                           double* bsum);
int mpdata_plan_level_hist_f32(mpdata_plan* plan, int64_t sl0, int64_t n, int tc, int nb, const double* edges, float* cnt,
                               float* bsum);
/* the same on instances [sl0, sl0+n) of a reference-layout DEVICE array f(ncrms,-2:nx+3,1,nzm,ntracers) (leading
 * dimension ncrms), which is only read; edges HOST; cnt, bsum as above (leading dimension n; bsum (n, nzm, nb, ntr)).
 * Asynchronous on `stream`; 64-bit offsets. */
int mpdata_level_hist_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, const double* f, int tc, int nb,
                             const double* edges, double* cnt, double* bsum, int first_tracer, int ntr, void* stream);
int mpdata_level_hist_f32_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, const float* f, int tc,
                                 int nb, const double* edges, float* cnt, float* bsum, int first_tracer, int ntr, void* stream);

/* ---- 3ac. Per-level updraft and downdraft sampling of a resident plan (the one block call that looks at a tracer and
 * the vertical velocity of a cell TOGETHER: 3g - 3ab reduce the tracers, 3h and 3j touch the velocities, none joins the two
 * halves of a plan's state.  The pair is what the statistics of a cloud-resolving model are built on: SAM's conditional
 * averages -- core, downdraft core, environment -- sample by the cell-centred w and a cloud condition; the same sampling
 * gives the cloudy and unsaturated up and down mass fluxes an MMF hands back to the global model every step, the in-core
 * means and the resolved flux w f split by draft).  This section is the specification; the reference tree has no such
 * routine.  For a condition tracer tc (tc = -1: no tracer condition), a range of value tracers [first_tracer, first_tracer
 * + ntracers) -- tc may lie inside it --, every instance sl in [sl0, sl0 + n) with b = sl - sl0, every level k = 1 .. nzm,
 * nzm = nz - 1, over the INTERIOR columns i = 1 .. nx, with c_i = f(sl,i,k,tc) and v_i = f(sl,i,k,first_tracer + j), every
 * statement below is rounded ONCE in the plan's precision, in this association, with nothing contracted, and the
 * comparisons are plain compare-and-select, so EXACT and FAST plans give the same bits:
 *   wk1  = w(sl,i,k+1) for k < nzm,  +0 for k = nzm        (as 3h: the caller's w(:,:,:,nz) is never read)
 *   a    = w(sl,i,k) + wk1 ;  wc = 0.5 * a                  (the cell-centred vertical velocity)
 *   in_i = tc < 0 ? true : (lo ? c_i > lo(b,k) : true) and (hi ? c_i <= hi(b,k) : true)          (exactly 3v)
 *   class of column i, only where in_i:   UP (0): wc > wup    DOWN (1): wc < wdn    ENV (2): otherwise
 *   cnt  (b,k,c)    :  q = +0;  do i = 1, nx:  if class_i == c:  q = q + 1
 *   wsum (b,k,c)    :  s = +0;  do i = 1, nx:  if class_i == c:  s = s + wc
 *   fsum (b,k,c,j)  :  s = +0;  do i = 1, nx:  if class_i == c:  s = s + v_i
 *   wfsum(b,k,c,j)  :  s = +0;  do i = 1, nx:  if class_i == c:  p = wc * v_i;  s = s + p
 * wup and wdn are doubles by value, each rounded once to the plan's precision (as c of 3p); wdn <= wup is required, +-inf
 * are allowed, so one-sided classes or no draft classes at all are a single call; wc == wup and wc == wdn are ENV.  A NaN
 * in w, c_i, lo or hi is outside the contract.  Selection means selection, as in 3v: a column outside a class contributes
 * nothing to it, whatever bits its value tracer holds -- no multiplication by a mask; a column that is not in_i is in no
 * class.  Sums are SUMS: the caller multiplies by rho and divides by cnt.  cnt is a real of the plan's precision and exact
 * (nx < 2^24): an implementation may count in integers and convert.
 * All four outputs are optional, at least one is required; lo and hi are optional, and with tc < 0 both must be NULL.  lo
 * and hi are (n, nzm), cnt and wsum (n, nzm, 3), fsum and wfsum (n, nzm, 3, ntracers): the plan's precision, reference
 * layout, the instance index fastest with leading dimension n (the block's first instance at index 0), then the level,
 * the class, the tracer -- the order of 3ab's cnt and bsum.  The tracer range is looked at only when fsum or wfsum is given.
 * Bit relations (they tie the call to 3g and 3v without passing through its own model):
 *   wup = +inf, wdn = -inf: cnt(:,:,ENV) and fsum(:,:,ENV,:) have the bits of 3v's cnt and csum with the same tc, lo, hi;
 *     UP and DOWN are +0 throughout.  With tc = -1 as well: fsum(:,:,ENV,:) has the bits of 3g's sum and cnt(:,:,ENV) = nx.
 *   any thresholds: cnt(UP) + cnt(DOWN) + cnt(ENV) equals 3v's cnt (all exact integers).
 * Towards the rest of a plan: nothing of the plan changes -- f, u, w, filled, have_u, have_w, the halo marks, the seam
 * marks, the timing pair and last_kernel_ms --; halo columns of f and w are never read, so a PERIODIC plan needs no wrap;
 * the call is outside the run's event pair.  The plan must hold w: after mpdata_plan_run_uw the call returns MPDATA_ESTATE
 * until w has been imported whole again; u is not needed -- a plan that holds w but not u works.
 *   windowed plans (3e, nz > 238) are supported: only OWNED levels are read, each with lo / hi of its tall level, each
 *     written to the tall level it stands for; no seam refresh is launched in front; wk1 is taken inside the window as 3h
 *     takes it and is +0 only at the tall top.
 *   no output is reached by the phantom half of an odd fp32 plan (3f), the partner of a split fp32 pair or a padding slot,
 *     and no byte outside the four outputs is touched.
 * A kernel of its own on every kind of plan (mpdata_level_draft.hip), not fused into the run.  Wave-major and windowed
 * plans: the lane-owned walk of 3v -- a lane owns one (instance, level) element, for fp32 both halves, and walks its
 * interior column slots as read-only linear streams; w(k) and w(k+1) are the two streams of 3h (element e + 1 through an
 * address and a column stride of its own); the value tracers lie at signed 64-bit offsets from the tc stream and are a loop
 * inside the kernel; every accumulator is lane-local in column order; no atomics, no cross-lane traffic, no LDS.  ONE form
 * at every nx: nothing of a column is kept between walks -- no class mask, no cached wc --, the class is formed again in
 * every walk from w(k), w(k+1) and c_i, and a walk carries a GROUP of 4, 2 or 1 value tracers (the most that is left, 8
 * or 4 columns in flight), so the three class streams are read once per group; the first walk also forms cnt and wsum.
 * The counters are 32-bit integers, made reals at the store.  Reference-layout plans and the array forms: one thread per
 * instance and level row, loops over i, 64-bit offsets, one value tracer a walk.
 * Checked before any device call, in this order -- a failed call changes nothing and launches nothing:
 * MPDATA_EINVAL: null plan, n < 1, a range outside [0, ncrms), tc outside [-1, ntracers), lo or hi given with tc < 0, a NaN
 * in wup or wdn, wdn > wup (checked on the doubles as given: rounding is monotone), all four outputs NULL, with fsum or
 * wfsum a tracer range that is empty or outside the plan; in the array forms bad sizes (ncrms < 1, nx < 1, nz < 2,
 * ntracers < 1), a block outside the arrays, a null w, a null f where tc >= 0, fsum or wfsum needs it, then the same list.
 * MPDATA_EUNSUPPORTED: a multi-GPU handle, as in 3d - 3ab (take mpdata_plan_shard_plan(plan, g) and a shard-local sl0).
 * MPDATA_ESTATE: a host form of the other precision; a plan never filled; a plan that does not hold w.
 * Time on the MI355X (docs/EXPERIMENTS.md AM, tools/level_draft_bench.py, profiles/level_draft_bench.json):
 * 65536 x 32 x 28, cold, plans of nine tracers, tc with lo and hi, wup = 0.25, wdn = -0.25 (6 % of the cells UP, 6 % DOWN, 38 %
 * ENV), the median of five rounds (their spread at most 1.5 %; the block of 64: 3.0 %), fp64 / fp32: cnt and wsum alone 0.255 /
 * 0.157 ms; fsum of 1, 3, 8 tracers 0.314 / 0.174, 0.631 / 0.349, 1.381 / 0.795 ms; fsum and wfsum of the same 0.349 / 0.204, 0.734 /
 * 0.467, 1.693 / 1.082 ms; a block of 64 instances (fsum and wfsum of 3) 0.021 / 0.031 ms.  Achieved on the algorithmic bytes (the
 * interior of w twice, of tc and the value tracers once): 5.3 / 4.3 TB/s for cnt and wsum, 5.8 / 5.2, 4.3 / 3.9, 3.6 / 3.1 TB/s for
 * fsum of 1, 3, 8 and 5.2 / 4.4, 3.7 / 2.9, 2.9 / 2.3 TB/s with wfsum (the two w streams overlap by all but one level, so the
 * bytes that reach memory are fewer).  Against (a) mpdata_plan_level_cond_device with the same tracers, one stream fewer:
 * cnt and wsum 2.43 x / 2.51 x its cnt; fsum 1.49 x, 1.59 x, 1.57 x / 1.52 x, 1.56 x, 1.60 x; with wfsum 1.66 x, 1.85 x, 1.92 x /
 * 1.78 x, 2.08 x, 2.18 x.  Against (b) mpdata_plan_courant_device, the same two w streams and u: cnt and wsum 1.18 x / 1.41 x.
 * Against (c) mpdata_plan_export_device of the T + 1 tracers, the old route, which still leaves the caller's kernel and their
 * copy of w: fsum 0.75 x, 0.76 x, 0.75 x / 0.82 x, 0.85 x, 0.88 x; with wfsum 0.83 x, 0.88 x, 0.92 x / 0.96 x, 1.13 x, 1.20 x.  Said
 * plainly: the call costs 1.5 x to 2.2 x a level_cond call on the same tracers -- the class is formed again in every walk and
 * every cell pays six selected adds per value tracer with wfsum --, cnt and wsum alone cost 2.4 x level_cond's cnt, and in fp32
 * with wfsum of three or more tracers it LOSES to the plain export of the tracers (1.13 x, 1.20 x).  4096 x 32 x 300 (6 windows;
 * spread at most 2.9 %): cnt and wsum 0.235 / 0.180 ms; fsum 0.260, 0.534, 1.141 / 0.157, 0.351, 0.711 ms; with wfsum 0.293, 0.647,
 * 1.416 / 0.210, 0.491, 1.065 ms; 1.44 x to 2.61 x level_cond; against the export fsum 0.81 x, 0.85 x, 0.81 x / 0.54 x, 0.62 x, 0.56 x,
 * with wfsum 0.92 x, 1.03 x (a loss), 1.01 x (unresolved) / 0.73 x, 0.86 x, 0.84 x.  The groups of 4, 2, 1 tracers a walk against
 * walks of one or of two at most: not measured. */
#define MPDATA_LEVEL_DRAFT_UP 0
#define MPDATA_LEVEL_DRAFT_DOWN 1
#define MPDATA_LEVEL_DRAFT_ENV 2
/* instances [sl0, sl0+n) of a resident plan; whole plan: sl0 = 0, n = ncrms.  lo, hi, cnt, wsum, fsum, wfsum: device arrays
 * of the plan's precision on the plan's device, asynchronous on the plan's stream. */
int mpdata_plan_level_draft_device(mpdata_plan* plan, int64_t sl0, int64_t n, int tc, const void* lo, const void* hi, double wup,
                                   double wdn, void* cnt, void* wsum, void* fsum, void* wfsum, int first_tracer, int ntracers);
/* host arrays, all tracers (fsum, wfsum (n, nzm, 3, ntracers of the plan)), synchronous (the plan's block staging buffer, as
 * the 3g - 3ab host forms) */
int mpdata_plan_level_draft(mpdata_plan* plan, int64_t sl0, int64_t n, int tc, const double* lo, const double* hi, double wup,
                            double wdn, double* cnt, double* wsum, double* fsum, double* wfsum);
int mpdata_plan_level_draft_f32(mpdata_plan* plan, int64_t sl0, int64_t n, int tc, const float* lo, const float* hi, double wup,
                                double wdn, float* cnt, float* wsum, float* fsum, float* wfsum);
/* the same on instances [sl0, sl0+n) of reference-layout DEVICE arrays f(ncrms,-2:nx+3,1,nzm,ntracers) and
 * w(ncrms,-1:nx+2,1,nz) (leading dimension ncrms), which are only read; w is required, f only where tc >= 0, fsum or wfsum
 * needs it; the outputs as above (leading dimension n).  Asynchronous on `stream`; 64-bit offsets. */
int mpdata_level_draft_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, const double* f, const double* w,
                              int tc, const double* lo, const double* hi, double wup, double wdn, double* cnt, double* wsum,
                              double* fsum, double* wfsum, int first_tracer, int ntr, void* stream);
int mpdata_level_draft_f32_device(int64_t ncrms, int nx, int nz, int ntracers, int64_t sl0, int64_t n, const float* f, const float* w,
                                  int tc, const float* lo, const float* hi, double wup, double wdn, float* cnt, float* wsum,
                                  float* fsum, float* wfsum, int first_tracer, int ntr, void* stream);

/* ---- 4. Synthetic inputs on the device (bench/tests; the reference's init,
 * :645-660, with a portable counter-based generator instead of the
 * compiler's random_number).  Fills `rows` x `nloc` doubles of array `sid`
 * (0..6 = adz,f,u,w,rho,rhow,flux) for CRM instances [sl0, sl0+nloc) of a
 * global problem of ncrms_global instances. dist: 1 conditioned, 2 raw
 * U[0,1), 3 raw with signed u,w. */
int mpdata_fill_synthetic_device(double* a, int sid, int64_t rows, int64_t ncrms_global,
                                 int64_t sl0, int64_t nloc, uint64_t seed, int dist,
                                 void* stream);

/* ---- 4b. A minimal device workspace for hosts that cannot call HIP themselves (the Fortran
 * driver's device-resident mode: the global arrays are generated on the root GPU with
 * mpdata_fill_synthetic_device and handed to mpdata_plan_import_device).  mpdata_device_sum: the sum
 * of the elements j < n with (j mod stride) < block (block = stride = n: all of them), in a fixed
 * order (a checksum, reproducible run to run). */
int mpdata_device_alloc(void** ptr, int64_t bytes);   /* on the current device */
/* ... on the device a plan takes full-width device arrays from: its own device; the ROOT GPU (shard
 * 0's device) of a multi-GPU plan.  mpdata_plan_import_device / _export_device / _run_uw on a
 * multi-GPU plan return MPDATA_EINVAL for an array that lives anywhere else. */
int mpdata_plan_device_alloc(mpdata_plan* plan, void** ptr, int64_t bytes);
int mpdata_device_free(void* ptr);
int mpdata_device_sum(const double* a, int64_t n, int64_t block, int64_t stride, double* sum);
/* (mpdata_fill_synthetic_device with a NULL stream and mpdata_device_sum run on the device the array
 * lives on, whatever the current device is.) */

/* ---- 5. Shard pack/unpack for the multi-GPU scatter/gather (device
 * pointers).  A shard [sl0, sl0+nloc) of an array with leading dimension
 * ncrms is a strided slab; pack makes it contiguous (leading dimension
 * nloc), unpack writes it back. */
int mpdata_pack_shard_device(const double* full, double* shard, int64_t rows, int64_t ncrms,
                             int64_t sl0, int64_t nloc, void* stream);
int mpdata_unpack_shard_device(double* full, const double* shard, int64_t rows, int64_t ncrms,
                               int64_t sl0, int64_t nloc, void* stream);

/* ---- 6. fp32: the reference's precision switch (`rp`, reference :12-13; note that the
 * `selected_real_kind(7)` it asks for is fp64 on conforming compilers -- IEEE single is
 * `selected_real_kind(6)`).  Same array contract with 4-byte reals.  Kernels cover nz <= 238
 * for even ncrms (two adjacent instances per lane, packed fp32 arithmetic; above 64 levels through
 * a wave-major plan, as the fp64 device call) and nz <= 32 for odd ncrms (section 3f, when switched on: the packed
 * kernels at every nz they cover).  EXACT variant: f bit-identical to an fp32 build of the reference. */
int mpdata_advect_scalar2d_f32(int64_t ncrms, int nx, int nz, int ntracers,
                               float* f, const float* u, const float* w,
                               const float* rho, const float* rhow,
                               const float* adz, float* flux);
int mpdata_advect_scalar2d_f32_device(int64_t ncrms, int nx, int nz, int ntracers,
                                      float* f, const float* u, const float* w,
                                      const float* rho, const float* rhow,
                                      const float* adz, float* flux, void* stream);
int mpdata_fill_synthetic_f32_device(float* a, int sid, int64_t rows, int64_t ncrms_global,
                                     int64_t sl0, int64_t nloc, uint64_t seed, int dist,
                                     void* stream);
int64_t mpdata_algorithmic_bytes_f32(int64_t ncrms, int nx, int nz, int ntracers);
/* fp32 plans: create / upload / download have _f32 forms; run, sync, last_kernel_ms and
 * destroy are the functions of section 3 (a plan remembers its precision; mixing the two
 * returns MPDATA_ESTATE). */
int mpdata_plan_create_f32(int64_t ncrms, int nx, int nz, int ntracers, mpdata_plan** plan);
int mpdata_plan_upload_f32(mpdata_plan* plan, const float* f, const float* u, const float* w,
                           const float* rho, const float* rhow, const float* adz,
                           const float* flux);
int mpdata_plan_download_f32(mpdata_plan* plan, float* f, float* flux);

/* ---- 7. Stage-by-stage debug mode (not a fast path).  The same routine as eight unfused
 * kernels, one per stage of the reference -- the split its OpenACC version makes, reference
 * :112-235 -- that materialise the reference's temporaries (:485-491) in caller-provided
 * device arrays uuu(ncrms,-1:nx+3,nzm), www(ncrms,-1:nx+2,nz), mx/mn(ncrms,0:nx+1,nzm), and
 * stop after stage `last_stage`:
 *   1 extrema of the incoming field (:513-526)   2 upwind fluxes + flux sum (:528-548)
 *   3 first-pass update (:550-560)               4 antidiffusive fluxes (:561-586)
 *   5 extrema of the first-pass field (:588-600) 6 limiter ratios (:601-612)
 *   7 limited fluxes, flux += (:613-627)         8 final update (:630-637)
 * Every array is then what the reference holds at that point, bit for bit (no FMA
 * contraction, reference expression and summation order), so a parity failure of the fused
 * kernels can be localised to a stage.  fp64, one tracer. */
int mpdata_debug_stages_device(int64_t ncrms, int nx, int nz, int last_stage, double* f,
                               const double* u, const double* w, const double* rho,
                               const double* rhow, const double* adz, double* flux,
                               double* uuu, double* www, double* mx, double* mn, void* stream);

/* ---- 8. Misc. */
int mpdata_set_variant(int variant);      /* MPDATA_VARIANT_*; returns previous */
int mpdata_get_variant(void);
/* Serpentine tile order of wave-major plans (every other run of a plan walks its tiles from the
 * other end and so starts on what the previous run left in the Infinity Cache; +2 % when
 * consecutive runs share u, w).  OFF by default (MPDATA_SERPENTINE=1 in the environment turns it
 * on); returns the previous setting. */
int mpdata_set_serpentine(int on);
/* Test switches of the wave-major launch (bit 0: the batch form of the kernel for one tracer as
 * well, bit 1: one tracer per wave in tracer batches, bit 2: an odd last tracer as a two-tracer
 * wave with an empty half, bit 3: an odd last tracer through a launch of its own behind the batch
 * -- the default takes it through one more wave per tile of the batch launch; MPDATA_WM_NOSTREAM /
 * MPDATA_WM_TPW1 / MPDATA_WM_NOSPLIT / MPDATA_WM_SPLIT in the environment set the initial value);
 * flags < 0 only queries.  Returns the previous value. */
int mpdata_set_wm_flags(int flags);
int mpdata_set_tile(int tile);            /* kernel tiling id; -1 = default */
int mpdata_set_debug_buffer(void* dev_ptr); /* diagnostic builds only (-DMPDWM_STAMPS): per-wave stamp buffer */
int mpdata_device_count(void);
int64_t mpdata_algorithmic_bytes(int64_t ncrms, int nx, int nz, int ntracers);
/* Diagnostic: GB/s this GPU sustains for the routine's traffic mix (3 arrays read, 1 written in
 * place) as a linear, aligned, 16-byte-per-lane stream; nontemporal = 1: streaming loads/stores. */
int mpdata_diag_stream_3r1w(int64_t bytes_per_array, int nontemporal, int iters, double* gbs);
const char* mpdata_last_error(void);
const char* mpdata_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MPDATA_HIP_H */
