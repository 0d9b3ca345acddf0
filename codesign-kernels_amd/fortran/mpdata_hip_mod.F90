!> Fortran face of libmpdata_hip.so (include/mpdata_hip.h): the thin
!! ISO_C_BINDING layer and the drop-in `advect_scalar2D(f,u,w,rho,rhow,flux)`.
!!
!! The dummy-argument list and the array shapes are those of the reference's
!! advect_scalar2D_cpu / _openacc_1 / _openacc_2
!! (mmf-mpdata-tracer/advect_scalar2D_pushncols_openacc.F90:477-484, :247, :72);
!! sizes and adz come from module mpdata_grid, where the reference takes them
!! by host association (:7-30).  The binding style (bind(C,name=..), scalars by
!! value, arrays as bare pointers, persistent device state behind the library)
!! follows the reference's own Fortran->C++ precedent, nested_loops/cke_mod.F90:4-50.
!! There is no CPU implementation behind this interface: a failing HIP call
!! stops the program.
module mpdata_hip_mod
  use iso_c_binding
  use mpdata_grid
  implicit none
  private
  public :: advect_scalar2D, advect_resident_begin, advect_resident_run, advect_resident_end
  public :: mpdata_set_variant, mpdata_check, advect_transfer_stats
  public :: advect_device_problem_run
  ! the plan API itself (include/mpdata_hip.h sections 3, 3b, 3d, 4, 4b): what a host model that keeps its own plan handle
  ! calls -- every block call below takes that handle
  public :: mpdata_advect_scalar2d_c, mpdata_plan_create_c, mpdata_plan_create_multi_c, mpdata_plan_upload_c
  public :: mpdata_plan_run_c, mpdata_plan_run_tracers_c, mpdata_plan_run_uw_c, mpdata_plan_sync_c, mpdata_plan_download_c
  public :: mpdata_plan_last_kernel_ms_c, mpdata_plan_set_timing_c, mpdata_plan_set_stream_c, mpdata_plan_destroy_c
  public :: mpdata_plan_import_device_c, mpdata_plan_export_device_c, mpdata_plan_transfer_stats_c, mpdata_plan_ranks_seen_c
  public :: mpdata_plan_import_instances_device_c, mpdata_plan_export_instances_device_c, mpdata_plan_download_instances_c
  public :: mpdata_device_alloc_c, mpdata_plan_device_alloc_c, mpdata_device_free_c, mpdata_device_sum_c
  public :: mpdata_fill_synthetic_device_c, mpdata_last_error_c
  ! periodic lateral boundaries (include/mpdata_hip.h sections 3a, 3c): the CRMs of the MMF are periodic in x
  public :: MPDATA_BOUNDARY_GIVEN, MPDATA_BOUNDARY_PERIODIC
  public :: mpdata_plan_set_boundary_c, mpdata_plan_boundary_c, mpdata_periodic_halo_device_c
  integer(c_int), parameter :: MPDATA_BOUNDARY_GIVEN = 0, MPDATA_BOUNDARY_PERIODIC = 1
  ! tall columns (include/mpdata_hip.h section 3e): plans with nz > 238 as overlapping level windows; the library also
  ! reads MPDATA_TALL_COLUMNS=1 from the environment, so a driver needs no call
  public :: mpdata_set_tall_columns_c, mpdata_plan_level_windows_c
  ! fp32 with an odd ncrms on the packed kernels (include/mpdata_hip.h section 3f); the library also reads
  ! MPDATA_F32_ODD_NCRMS=1 from the environment, so a driver needs no call
  public :: mpdata_set_f32_odd_ncrms_c
  ! horizontal sum / min / max per level of a resident plan's tracers (include/mpdata_hip.h section 3g)
  public :: mpdata_plan_level_stats_device_c, mpdata_plan_level_stats_c, mpdata_level_stats_device_c

  ! outflow Courant number of a resident plan's velocities (include/mpdata_hip.h section 3h)
  public :: mpdata_plan_courant_device_c, mpdata_plan_courant_device, mpdata_plan_courant_c, mpdata_courant_device_c
  ! per-level increments of a resident plan's tracers, in place (include/mpdata_hip.h section 3i)
  public :: mpdata_plan_level_add_device_c, mpdata_plan_level_add_c, mpdata_level_add_device_c
  integer(c_int), parameter, public :: MPDATA_LEVEL_ADD = 0, MPDATA_LEVEL_ADD_CLIP = 1
  ! one factor per instance on a resident plan's u and w, in place (include/mpdata_hip.h section 3j)
  public :: mpdata_plan_scale_uw_device_c, mpdata_plan_scale_uw_c, mpdata_scale_uw_device_c
  ! mass-weighted column integrals of a resident plan's tracers (include/mpdata_hip.h section 3k)
  public :: mpdata_plan_column_path_device_c, mpdata_plan_column_path_c, mpdata_column_path_device_c
  ! eddy diffusion of a resident plan's tracers, in place (include/mpdata_hip.h section 3l)
  public :: mpdata_plan_diffuse_device_c, mpdata_plan_diffuse_c, mpdata_diffuse_device_c
  ! large-scale vertical advection of a resident plan's tracers, in place (include/mpdata_hip.h section 3m): the device
  ! form only -- it carries no reals of its own, so one binding serves both precisions; the per-precision host and array
  ! forms (mpdata_plan_subside[_f32], mpdata_subside[_f32]_device) have no Fortran interface yet
  public :: mpdata_plan_subside_device_c
  ! sedimentation of a resident plan's tracers, in place (include/mpdata_hip.h section 3n): the device form only, one
  ! binding for both precisions as for 3m; mpdata_plan_sediment[_f32] and mpdata_sediment[_f32]_device have no Fortran
  ! interface yet
  public :: mpdata_plan_sediment_device_c
  ! implicit vertical solve of a resident plan's tracers, in place (include/mpdata_hip.h section 3o): the device form only,
  ! one binding for both precisions as for 3m / 3n; mpdata_plan_vsolve[_f32] and mpdata_vsolve[_f32]_device have no
  ! Fortran interface yet
  public :: mpdata_plan_vsolve_device_c
  ! per-cell sources of a resident plan's tracers, in place (include/mpdata_hip.h section 3p): the device form only, one
  ! binding for both precisions -- its one real, the factor c, is a double in C for both; mpdata_plan_cell_add[_f32] and
  ! mpdata_cell_add[_f32]_device have no Fortran interface yet
  public :: mpdata_plan_cell_add_device_c
  integer(c_int), parameter, public :: MPDATA_CELL_ADD = 0, MPDATA_CELL_ADD_CLIP = 1
  ! fused column step of a resident plan's tracers, in place (include/mpdata_hip.h section 3q): the device form only, one
  ! binding for both precisions, next to 3p's in the interface block of the bindings with a real by value;
  ! mpdata_plan_column_step[_f32] and mpdata_column_step[_f32]_device have no Fortran interface yet
  public :: mpdata_plan_column_step_device_c
  ! relaxation of a resident plan's tracers to a level profile, in place (include/mpdata_hip.h section 3r): the device form
  ! only, one binding for both precisions -- it carries no reals of its own; it stands in the second interface block, next
  ! to 3p's and 3q's; mpdata_plan_relax[_f32] and mpdata_relax[_f32]_device have no Fortran interface yet
  public :: mpdata_plan_relax_device_c
  ! first-order conversion between two tracers of a resident plan, in place (include/mpdata_hip.h section 3t): the device
  ! form only, one binding for both precisions -- it carries no reals of its own; it stands in the second interface block,
  ! behind 3r's; mpdata_plan_convert[_f32] and mpdata_convert[_f32]_device have no Fortran interface yet
  public :: mpdata_plan_convert_device_c
  integer(c_int), parameter, public :: MPDATA_CONVERT_LIMIT = 1
  ! per-level covariance of two tracers of a resident plan (include/mpdata_hip.h section 3u): the device form only, one
  ! binding for both precisions -- it carries no reals of its own; it stands in the second interface block, behind 3t's;
  ! mpdata_plan_level_cov[_f32] and mpdata_level_cov[_f32]_device have no Fortran interface yet
  public :: mpdata_plan_level_cov_device_c
  integer(c_int), parameter, public :: MPDATA_LEVEL_COV_RAW = 1
  ! per-level conditional counts and sums of a resident plan's tracers (include/mpdata_hip.h section 3v): the device form
  ! only, one binding for both precisions -- it carries no reals of its own; it stands in the second interface block,
  ! behind 3u's; mpdata_plan_level_cond[_f32] and mpdata_level_cond[_f32]_device have no Fortran interface yet
  public :: mpdata_plan_level_cond_device_c
  ! per-column conditional level counts, tops and paths of a resident plan's tracers (include/mpdata_hip.h section 3w): all
  ! five entry points, each bound by its literal name -- the arrays are c_ptr, so the fp64 and the fp32 form of the host
  ! and of the array call are two interfaces each and a caller picks by its precision (tests/fortran/column_cond_calls.F90);
  ! they stand in the second interface block, behind 3v's
  public :: mpdata_plan_column_cond_device_c, mpdata_plan_column_cond_c, mpdata_plan_column_cond_f32_c
  public :: mpdata_column_cond_device_c, mpdata_column_cond_f32_device_c
  ! conservative per-level non-negativity fixer of a resident plan's tracers, in place (include/mpdata_hip.h section 3x): all
  ! five entry points, each bound by its literal name as 3w's are (tests/fortran/nonneg_calls.F90); they stand in the second
  ! interface block, behind 3w's
  public :: mpdata_plan_nonneg_device_c, mpdata_plan_nonneg_c, mpdata_plan_nonneg_f32_c
  public :: mpdata_nonneg_device_c, mpdata_nonneg_f32_device_c
  ! saturation adjustment of a resident plan's tracers, in place (include/mpdata_hip.h section 3y): the derived type of the
  ! caller's numbers (struct mpdata_satadj_params, passed as c_loc of a target variable) and all five entry points, each
  ! bound by its literal name as 3x's are (tests/fortran/satadj_calls.F90); they stand in the second interface block,
  ! behind 3x's
  public :: mpdata_satadj_params
  public :: mpdata_plan_satadj_device_c, mpdata_plan_satadj_c, mpdata_plan_satadj_f32_c
  public :: mpdata_satadj_device_c, mpdata_satadj_f32_device_c
  integer(c_int), parameter, public :: MPDATA_SATADJ_ICE = 1
  type, bind(C) :: mpdata_satadj_params
    real(c_double) :: esw(9), desw(9)   ! liquid: es(x), d es / dT (x), degree-8 polynomials in x, esw(1) the constant term
    real(c_double) :: esi(9), desi(9)   ! ice: the same; read only with MPDATA_SATADJ_ICE
    real(c_double) :: t0, xmin          ! x = T - t0, bounded below by xmin
    real(c_double) :: eps               ! qs = (eps * es) / max(es, p - es)
    real(c_double) :: lv, ls            ! L / cp of condensation and of sublimation
    real(c_double) :: tmin, tmax        ! the mixed-phase ramp, tmin < tmax; ICE only
    real(c_double) :: tol               ! Newton stops when |dT| <= tol ...
    integer(c_int) :: maxit             ! ... or after maxit steps, 1 <= maxit <= 32
  end type
  ! linear combinations of a resident plan's tracers, in place (include/mpdata_hip.h section 3z): all five entry points,
  ! each bound by its literal name as 3y's are (tests/fortran/combine_calls.F90); src is c_loc of an integer(c_int) array
  ! of the HOST in every form; they stand in the second interface block, behind 3y's
  public :: mpdata_plan_combine_device_c, mpdata_plan_combine_c, mpdata_plan_combine_f32_c
  public :: mpdata_combine_device_c, mpdata_combine_f32_device_c
  integer(c_int), parameter, public :: MPDATA_COMBINE_CLIP = 1
  integer(c_int), parameter, public :: MPDATA_COMBINE_MAX = 8
  ! running column integrals of a resident plan's tracers, in place (include/mpdata_hip.h section 3aa): all five entry
  ! points, each bound by its literal name as 3z's are (tests/fortran/column_scan_calls.F90); they stand in the second
  ! interface block, behind 3z's
  public :: mpdata_plan_column_scan_device_c, mpdata_plan_column_scan_c, mpdata_plan_column_scan_f32_c
  public :: mpdata_column_scan_device_c, mpdata_column_scan_f32_device_c
  ! per-level histograms of a resident plan's tracers (include/mpdata_hip.h section 3ab): all five entry points, each bound
  ! by its literal name as 3aa's are (tests/fortran/level_hist_calls.F90); they stand in the second interface block, behind
  ! 3aa's.  edges is a HOST array of real(c_double) in every form
  public :: mpdata_plan_level_hist_device_c, mpdata_plan_level_hist_c, mpdata_plan_level_hist_f32_c
  public :: mpdata_level_hist_device_c, mpdata_level_hist_f32_device_c
  integer(c_int), parameter, public :: MPDATA_LEVEL_HIST_MAX_BINS = 32
  ! per-level updraft / downdraft sampling of a resident plan (include/mpdata_hip.h section 3ac): all five entry points,
  ! each bound by its literal name as 3ab's are (tests/fortran/level_draft_calls.F90); they stand in the second interface
  ! block, behind 3ab's.  wup and wdn are real(c_double) by value in every form
  public :: mpdata_plan_level_draft_device_c, mpdata_plan_level_draft_c, mpdata_plan_level_draft_f32_c
  public :: mpdata_level_draft_device_c, mpdata_level_draft_f32_device_c
  integer(c_int), parameter, public :: MPDATA_LEVEL_DRAFT_UP = 0
  integer(c_int), parameter, public :: MPDATA_LEVEL_DRAFT_DOWN = 1
  integer(c_int), parameter, public :: MPDATA_LEVEL_DRAFT_ENV = 2
  integer(c_int), parameter, public :: MPDATA_COLUMN_SCAN_DOWN = 1
  integer(c_int), parameter, public :: MPDATA_COLUMN_SCAN_EXCLUSIVE = 2
  ! implicit vertical diffusion of a resident plan's tracers with a per-cell diffusivity, in place (include/mpdata_hip.h
  ! section 3s): the device form only, one binding for both precisions as for 3o, next to it in the first interface block;
  ! mpdata_plan_vdiffuse[_f32] and mpdata_vdiffuse[_f32]_device have no Fortran interface yet
  public :: mpdata_plan_vdiffuse_device_c
  ! the C entry points that carry reals exist per precision (include/mpdata_hip.h sections 1-3
  ! and 6); `make single=1` (-DMPDATA_SINGLE) binds the fp32 ones, rp = c_float
#ifdef MPDATA_SINGLE
#define MPDATA_C_ADVECT "mpdata_advect_scalar2d_f32"
#define MPDATA_C_PLAN_CREATE "mpdata_plan_create_f32"
#define MPDATA_C_PLAN_UPLOAD "mpdata_plan_upload_f32"
#define MPDATA_C_PLAN_DOWNLOAD "mpdata_plan_download_f32"
#define MPDATA_C_PERIODIC_HALO "mpdata_periodic_halo_f32_device"
#define MPDATA_C_PLAN_DOWNLOAD_INSTANCES "mpdata_plan_download_instances_f32"
#define MPDATA_C_PLAN_LEVEL_STATS "mpdata_plan_level_stats_f32"
#define MPDATA_C_LEVEL_STATS_DEVICE "mpdata_level_stats_f32_device"
#define MPDATA_C_PLAN_COURANT "mpdata_plan_courant_f32"
#define MPDATA_C_COURANT_DEVICE "mpdata_courant_f32_device"
#define MPDATA_C_PLAN_LEVEL_ADD "mpdata_plan_level_add_f32"
#define MPDATA_C_LEVEL_ADD_DEVICE "mpdata_level_add_f32_device"
#define MPDATA_C_PLAN_SCALE_UW "mpdata_plan_scale_uw_f32"
#define MPDATA_C_SCALE_UW_DEVICE "mpdata_scale_uw_f32_device"
#define MPDATA_C_PLAN_COLUMN_PATH "mpdata_plan_column_path_f32"
#define MPDATA_C_COLUMN_PATH_DEVICE "mpdata_column_path_f32_device"
#define MPDATA_C_PLAN_DIFFUSE "mpdata_plan_diffuse_f32"
#define MPDATA_C_DIFFUSE_DEVICE "mpdata_diffuse_f32_device"
#else
#define MPDATA_C_ADVECT "mpdata_advect_scalar2d"
#define MPDATA_C_PLAN_CREATE "mpdata_plan_create"
#define MPDATA_C_PLAN_UPLOAD "mpdata_plan_upload"
#define MPDATA_C_PLAN_DOWNLOAD "mpdata_plan_download"
#define MPDATA_C_PERIODIC_HALO "mpdata_periodic_halo_device"
#define MPDATA_C_PLAN_DOWNLOAD_INSTANCES "mpdata_plan_download_instances"
#define MPDATA_C_PLAN_LEVEL_STATS "mpdata_plan_level_stats"
#define MPDATA_C_LEVEL_STATS_DEVICE "mpdata_level_stats_device"
#define MPDATA_C_PLAN_COURANT "mpdata_plan_courant"
#define MPDATA_C_COURANT_DEVICE "mpdata_courant_device"
#define MPDATA_C_PLAN_LEVEL_ADD "mpdata_plan_level_add"
#define MPDATA_C_LEVEL_ADD_DEVICE "mpdata_level_add_device"
#define MPDATA_C_PLAN_SCALE_UW "mpdata_plan_scale_uw"
#define MPDATA_C_SCALE_UW_DEVICE "mpdata_scale_uw_device"
#define MPDATA_C_PLAN_COLUMN_PATH "mpdata_plan_column_path"
#define MPDATA_C_COLUMN_PATH_DEVICE "mpdata_column_path_device"
#define MPDATA_C_PLAN_DIFFUSE "mpdata_plan_diffuse"
#define MPDATA_C_DIFFUSE_DEVICE "mpdata_diffuse_device"
#endif

  interface
    integer(c_int) function mpdata_advect_scalar2d_c(ncrms, nx, nz, ntracers, f, u, w, rho, rhow, adz, flux) &
        bind(C, name=MPDATA_C_ADVECT)
      import :: c_int, c_int64_t, rp
      integer(c_int64_t), value :: ncrms
      integer(c_int), value :: nx, nz, ntracers
      real(rp) :: f(*), flux(*)
      real(rp), intent(in) :: u(*), w(*), rho(*), rhow(*), adz(*)
    end function
    integer(c_int) function mpdata_plan_create_c(ncrms, nx, nz, ntracers, plan) bind(C, name=MPDATA_C_PLAN_CREATE)
      import :: c_int, c_int64_t, c_ptr
      integer(c_int64_t), value :: ncrms
      integer(c_int), value :: nx, nz, ntracers
      type(c_ptr) :: plan
    end function
    integer(c_int) function mpdata_plan_create_multi_c(ncrms, nx, nz, ntracers, ngpus, plan) &
        bind(C, name="mpdata_plan_create_multi")
      import :: c_int, c_int64_t, c_ptr
      integer(c_int64_t), value :: ncrms
      integer(c_int), value :: nx, nz, ntracers, ngpus
      type(c_ptr) :: plan
    end function
    integer(c_int) function mpdata_plan_transfer_stats_c(plan, scatter_s, gather_s, scatter_bytes_per_peer, gather_bytes_per_peer, &
        transport) &
        bind(C, name="mpdata_plan_transfer_stats")
      import :: c_int, c_int64_t, c_ptr, c_double
      type(c_ptr), value :: plan
      real(c_double) :: scatter_s, gather_s
      integer(c_int64_t) :: scatter_bytes_per_peer, gather_bytes_per_peer
      integer(c_int) :: transport
    end function
    integer(c_int) function mpdata_plan_upload_c(plan, f, u, w, rho, rhow, adz, flux) bind(C, name=MPDATA_C_PLAN_UPLOAD)
      import :: c_int, c_ptr, rp
      type(c_ptr), value :: plan
      real(rp), intent(in) :: f(*), u(*), w(*), rho(*), rhow(*), adz(*), flux(*)
    end function
    integer(c_int) function mpdata_plan_run_c(plan) bind(C, name="mpdata_plan_run")
      import :: c_int, c_ptr
      type(c_ptr), value :: plan
    end function
    ! a sub-range of the tracers
    integer(c_int) function mpdata_plan_run_tracers_c(plan, first_tracer, ntracers) bind(C, name="mpdata_plan_run_tracers")
      import :: c_int, c_ptr
      type(c_ptr), value :: plan
      integer(c_int), value :: first_tracer, ntracers
    end function
    ! one step on fresh reference-layout DEVICE u, w of the plan's precision; the plan holds no velocities afterwards
    integer(c_int) function mpdata_plan_run_uw_c(plan, first_tracer, ntracers, u, w) bind(C, name="mpdata_plan_run_uw")
      import :: c_int, c_ptr
      type(c_ptr), value :: plan
      integer(c_int), value :: first_tracer, ntracers
      type(c_ptr), value :: u, w
    end function
    integer(c_int) function mpdata_plan_sync_c(plan) bind(C, name="mpdata_plan_sync")
      import :: c_int, c_ptr
      type(c_ptr), value :: plan
    end function
    integer(c_int) function mpdata_plan_download_c(plan, f, flux) bind(C, name=MPDATA_C_PLAN_DOWNLOAD)
      import :: c_int, c_ptr, rp
      type(c_ptr), value :: plan
      real(rp) :: f(*), flux(*)
    end function
    integer(c_int) function mpdata_plan_last_kernel_ms_c(plan, ms) bind(C, name="mpdata_plan_last_kernel_ms")
      import :: c_int, c_ptr, c_double
      type(c_ptr), value :: plan
      real(c_double) :: ms
    end function
    ! on = 0: no event pair around the runs (mpdata_plan_last_kernel_ms_c then returns MPDATA_ESTATE)
    integer(c_int) function mpdata_plan_set_timing_c(plan, on) bind(C, name="mpdata_plan_set_timing")
      import :: c_int, c_ptr
      type(c_ptr), value :: plan
      integer(c_int), value :: on
    end function
    ! run on the caller's stream (a hipStream_t; c_null_ptr: the default stream) from now on
    integer(c_int) function mpdata_plan_set_stream_c(plan, stream) bind(C, name="mpdata_plan_set_stream")
      import :: c_int, c_ptr
      type(c_ptr), value :: plan, stream
    end function
    integer(c_int) function mpdata_plan_destroy_c(plan) bind(C, name="mpdata_plan_destroy")
      import :: c_int, c_ptr
      type(c_ptr), value :: plan
    end function
    integer(c_int) function mpdata_set_variant(variant) bind(C, name="mpdata_set_variant")
      import :: c_int
      integer(c_int), value :: variant
    end function
    type(c_ptr) function mpdata_last_error_c() bind(C, name="mpdata_last_error")
      import :: c_ptr
    end function
    ! ---- device-resident mode: the global arrays live on the root GPU (include/mpdata_hip.h 3, 3b, 4, 4b)
    integer(c_int) function mpdata_device_alloc_c(ptr, bytes) bind(C, name="mpdata_device_alloc")
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr) :: ptr
      integer(c_int64_t), value :: bytes
    end function
    integer(c_int) function mpdata_plan_device_alloc_c(plan, ptr, bytes) bind(C, name="mpdata_plan_device_alloc")
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: plan
      type(c_ptr) :: ptr
      integer(c_int64_t), value :: bytes
    end function
    integer(c_int) function mpdata_device_free_c(ptr) bind(C, name="mpdata_device_free")
      import :: c_int, c_ptr
      type(c_ptr), value :: ptr
    end function
    integer(c_int) function mpdata_device_sum_c(a, n, block, stride, sum) bind(C, name="mpdata_device_sum")
      import :: c_int, c_int64_t, c_ptr, c_double
      type(c_ptr), value :: a
      integer(c_int64_t), value :: n, block, stride
      real(c_double) :: sum
    end function
    integer(c_int) function mpdata_fill_synthetic_device_c(a, sid, rows, ncrms_global, sl0, nloc, seed, dist, stream) &
        bind(C, name="mpdata_fill_synthetic_device")
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: a, stream
      integer(c_int), value :: sid, dist
      integer(c_int64_t), value :: rows, ncrms_global, sl0, nloc, seed
    end function
    integer(c_int) function mpdata_plan_import_device_c(plan, f, u, w, rho, rhow, adz, flux, first_tracer, ntracers) &
        bind(C, name="mpdata_plan_import_device")
      import :: c_int, c_ptr
      type(c_ptr), value :: plan, f, u, w, rho, rhow, adz, flux
      integer(c_int), value :: first_tracer, ntracers
    end function
    integer(c_int) function mpdata_plan_export_device_c(plan, f, flux, first_tracer, ntracers) &
        bind(C, name="mpdata_plan_export_device")
      import :: c_int, c_ptr
      type(c_ptr), value :: plan, f, flux
      integer(c_int), value :: first_tracer, ntracers
    end function
    ! ---- blocks of CRM instances [sl0, sl0+n) of a filled plan (include/mpdata_hip.h 3d; sl0 counts from 0): reference-layout
    ! arrays of a problem of n instances (leading dimension n); device forms asynchronous (c_null_ptr: skipped), the
    ! host form synchronous and over all tracers
    integer(c_int) function mpdata_plan_import_instances_device_c(plan, sl0, n, f, u, w, rho, rhow, adz, flux, first_tracer, &
        ntracers) &
        bind(C, name="mpdata_plan_import_instances_device")
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: plan, f, u, w, rho, rhow, adz, flux
      integer(c_int64_t), value :: sl0, n
      integer(c_int), value :: first_tracer, ntracers
    end function
    integer(c_int) function mpdata_plan_export_instances_device_c(plan, sl0, n, f, flux, first_tracer, ntracers) &
        bind(C, name="mpdata_plan_export_instances_device")
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: plan, f, flux
      integer(c_int64_t), value :: sl0, n
      integer(c_int), value :: first_tracer, ntracers
    end function
    integer(c_int) function mpdata_plan_download_instances_c(plan, sl0, n, f, flux) &
        bind(C, name=MPDATA_C_PLAN_DOWNLOAD_INSTANCES)
      import :: c_int, c_int64_t, c_ptr, rp
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      real(rp) :: f(*), flux(*)
    end function
    integer(c_int) function mpdata_plan_ranks_seen_c(plan) bind(C, name="mpdata_plan_ranks_seen")
      import :: c_int, c_ptr
      type(c_ptr), value :: plan
    end function
    ! mode: MPDATA_BOUNDARY_GIVEN (default) or MPDATA_BOUNDARY_PERIODIC; returns 0 or MPDATA_EINVAL (-1)
    integer(c_int) function mpdata_plan_set_boundary_c(plan, mode) bind(C, name="mpdata_plan_set_boundary")
      import :: c_int, c_ptr
      type(c_ptr), value :: plan
      integer(c_int), value :: mode
    end function
    integer(c_int) function mpdata_plan_boundary_c(plan) bind(C, name="mpdata_plan_boundary")
      import :: c_int, c_ptr
      type(c_ptr), value :: plan
    end function
    ! on = 1: new plans with nz > 238 become windowed plans; returns the previous setting
    integer(c_int) function mpdata_set_tall_columns_c(on) bind(C, name="mpdata_set_tall_columns")
      import :: c_int
      integer(c_int), value :: on
    end function
    ! on = 1: fp32 plans and calls with an odd ncrms run on the packed kernels; returns the previous setting
    integer(c_int) function mpdata_set_f32_odd_ncrms_c(on) bind(C, name="mpdata_set_f32_odd_ncrms")
      import :: c_int
      integer(c_int), value :: on
    end function
    ! W, the level windows of a plan's columns (1: not a windowed plan)
    integer(c_int) function mpdata_plan_level_windows_c(plan) bind(C, name="mpdata_plan_level_windows")
      import :: c_int, c_ptr
      type(c_ptr), value :: plan
    end function
    ! reference-layout DEVICE arrays (c_null_ptr: skipped) made periodic in x, in place, on `stream`
    integer(c_int) function mpdata_periodic_halo_device_c(ncrms, nx, nz, ntracers, f, u, w, stream) &
        bind(C, name=MPDATA_C_PERIODIC_HALO)
      import :: c_int, c_int64_t, c_ptr
      integer(c_int64_t), value :: ncrms
      integer(c_int), value :: nx, nz, ntracers
      type(c_ptr), value :: f, u, w, stream
    end function
    ! section 3g: sum / min / max over the interior columns of f per instance, level and tracer; outputs (n, nzm [, ntracers]),
    ! c_null_ptr (host form: not possible, pass all three) = skipped.  Device arrays of the plan's precision, asynchronous:
    integer(c_int) function mpdata_plan_level_stats_device_c(plan, sl0, n, sum, mn, mx, first_tracer, ntracers) &
        bind(C, name="mpdata_plan_level_stats_device")
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      type(c_ptr), value :: sum, mn, mx
      integer(c_int), value :: first_tracer, ntracers
    end function
    ! host arrays, all tracers, synchronous
    integer(c_int) function mpdata_plan_level_stats_c(plan, sl0, n, sum, mn, mx) bind(C, name=MPDATA_C_PLAN_LEVEL_STATS)
      import :: c_int, c_int64_t, c_ptr, rp
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      real(rp) :: sum(*), mn(*), mx(*)
    end function
    ! the same reduction on a reference-layout device array f
    integer(c_int) function mpdata_level_stats_device_c(ncrms, nx, nz, ntracers, f, sum, mn, mx, stream) &
        bind(C, name=MPDATA_C_LEVEL_STATS_DEVICE)
      import :: c_int, c_int64_t, c_ptr
      integer(c_int64_t), value :: ncrms
      integer(c_int), value :: nx, nz, ntracers
      type(c_ptr), value :: f, sum, mn, mx, stream
    end function
    ! section 3h: outflow Courant number of the velocities the plan holds, instances [sl0, sl0+n): clev(n, nzm) the max over
    ! the interior columns per level, cinst(n) its max over the levels; device arrays of the plan's precision, c_null_ptr =
    ! skipped (not both), asynchronous on the plan's stream
    integer(c_int) function mpdata_plan_courant_device_c(plan, sl0, n, clev, cinst) bind(C, name="mpdata_plan_courant_device")
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      type(c_ptr), value :: clev, cinst
    end function
    ! host clev, cinst (c_loc of an array of the module's precision, or c_null_ptr: skipped, not both), synchronous: what a
    ! Fortran loop forms ncycle from
    integer(c_int) function mpdata_plan_courant_c(plan, sl0, n, clev, cinst) bind(C, name=MPDATA_C_PLAN_COURANT)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      type(c_ptr), value :: clev, cinst
    end function
    ! the same reduction on reference-layout device arrays u, w, rho(ncrms,nzm), adz(ncrms,nzm): the fresh u, w of a
    ! caller of mpdata_plan_run_uw_c
    integer(c_int) function mpdata_courant_device_c(ncrms, nx, nz, u, w, rho, adz, clev, cinst, stream) &
        bind(C, name=MPDATA_C_COURANT_DEVICE)
      import :: c_int, c_int64_t, c_ptr
      integer(c_int64_t), value :: ncrms
      integer(c_int), value :: nx, nz
      type(c_ptr), value :: u, w, rho, adz, clev, cinst
      type(c_ptr), value :: stream
    end function
    ! section 3i: f(sl,i,k,t) = f(sl,i,k,t) + d(sl,k,t) on every column i = -2 .. nx+3 of instances [sl0, sl0+n), in place
    ! (mode MPDATA_LEVEL_ADD_CLIP: max(0, .) of the sum); d(n, nzm [, ntracers]) -- the shape of a 3g output -- is only read.
    ! d a device array of the plan's precision, asynchronous on the plan's stream:
    integer(c_int) function mpdata_plan_level_add_device_c(plan, sl0, n, d, mode, first_tracer, ntracers) &
        bind(C, name="mpdata_plan_level_add_device")
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      type(c_ptr), value :: d
      integer(c_int), value :: mode, first_tracer, ntracers
    end function
    ! host d, all tracers, synchronous
    integer(c_int) function mpdata_plan_level_add_c(plan, sl0, n, d, mode) bind(C, name=MPDATA_C_PLAN_LEVEL_ADD)
      import :: c_int, c_int64_t, c_ptr, rp
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      real(rp), intent(in) :: d(*)
      integer(c_int), value :: mode
    end function
    ! the same on a reference-layout device array f with a device array d(ncrms, nzm [, ntracers])
    integer(c_int) function mpdata_level_add_device_c(ncrms, nx, nz, ntracers, f, d, mode, stream) &
        bind(C, name=MPDATA_C_LEVEL_ADD_DEVICE)
      import :: c_int, c_int64_t, c_ptr
      integer(c_int64_t), value :: ncrms
      integer(c_int), value :: nx, nz, ntracers
      type(c_ptr), value :: f, d
      integer(c_int), value :: mode
      type(c_ptr), value :: stream
    end function
    ! section 3j: u(sl,:,:) = u(sl,:,:) * su(sl-sl0+1), w(sl,:,:) = w(sl,:,:) * sw(sl-sl0+1) on every column and level of
    ! instances [sl0, sl0+n), in place; su(n), sw(n) are only read, c_null_ptr leaves that array as it is.
    ! su, sw device arrays of the plan's precision, asynchronous on the plan's stream:
    integer(c_int) function mpdata_plan_scale_uw_device_c(plan, sl0, n, su, sw) bind(C, name="mpdata_plan_scale_uw_device")
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      type(c_ptr), value :: su, sw
    end function
    ! host su, sw (c_loc of an array of the module's precision, or c_null_ptr), synchronous
    integer(c_int) function mpdata_plan_scale_uw_c(plan, sl0, n, su, sw) bind(C, name=MPDATA_C_PLAN_SCALE_UW)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      type(c_ptr), value :: su, sw
    end function
    ! the same on reference-layout device arrays u, w with device arrays su(ncrms), sw(ncrms); u or w may be c_null_ptr
    ! together with its factor
    integer(c_int) function mpdata_scale_uw_device_c(ncrms, nx, nz, u, w, su, sw, stream) bind(C, name=MPDATA_C_SCALE_UW_DEVICE)
      import :: c_int, c_int64_t, c_ptr
      integer(c_int64_t), value :: ncrms
      integer(c_int), value :: nx, nz
      type(c_ptr), value :: u, w, su, sw
      type(c_ptr), value :: stream
    end function
    ! ---- mass-weighted column integrals (include/mpdata_hip.h section 3k): path(n, nx [, ntracers]) = the sequential sum
    ! over k of (rho * adz) * f on the interior columns, mass(n [, ntracers]) = its sequential sum over i (c_null_ptr: skipped)
    ! device arrays of the plan's precision, asynchronous on the plan's stream:
    integer(c_int) function mpdata_plan_column_path_device_c(plan, sl0, n, path, mass, first_tracer, ntracers) &
        bind(C, name="mpdata_plan_column_path_device")
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      type(c_ptr), value :: path, mass
      integer(c_int), value :: first_tracer, ntracers
    end function
    ! host arrays, all tracers (c_loc of an array of the module's precision; mass may be c_null_ptr), synchronous
    integer(c_int) function mpdata_plan_column_path_c(plan, sl0, n, path, mass) bind(C, name=MPDATA_C_PLAN_COLUMN_PATH)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      type(c_ptr), value :: path, mass
    end function
    ! the same on reference-layout device arrays f, rho(ncrms,nzm), adz(ncrms,nzm)
    integer(c_int) function mpdata_column_path_device_c(ncrms, nx, nz, ntracers, f, rho, adz, path, mass, stream) &
        bind(C, name=MPDATA_C_COLUMN_PATH_DEVICE)
      import :: c_int, c_int64_t, c_ptr
      integer(c_int64_t), value :: ncrms
      integer(c_int), value :: nx, nz, ntracers
      type(c_ptr), value :: f, rho, adz, path, mass
      type(c_ptr), value :: stream
    end function
    ! ---- eddy diffusion of f in place (include/mpdata_hip.h section 3l): tkh(n, 0:nx+1, nzm), cx, cz(n, nzm), sb, st(n, nx)
    ! (c_null_ptr: zero flux), zflux(n, nz [, ntracers]) (c_null_ptr: skipped); windowed plans: MPDATA_EUNSUPPORTED
    ! device arrays of the plan's precision, asynchronous on the plan's stream:
    integer(c_int) function mpdata_plan_diffuse_device_c(plan, sl0, n, tkh, cx, cz, sb, st, zflux, first_tracer, ntracers) &
        bind(C, name="mpdata_plan_diffuse_device")
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      type(c_ptr), value :: tkh, cx, cz, sb, st, zflux
      integer(c_int), value :: first_tracer, ntracers
    end function
    ! host arrays, all tracers (c_loc of an array of the module's precision), synchronous
    integer(c_int) function mpdata_plan_diffuse_c(plan, sl0, n, tkh, cx, cz, sb, st, zflux) bind(C, name=MPDATA_C_PLAN_DIFFUSE)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      type(c_ptr), value :: tkh, cx, cz, sb, st, zflux
    end function
    ! the same on instances [sl0, sl0 + n) of reference-layout device arrays f, rho(ncrms,nzm), adz(ncrms,nzm)
    integer(c_int) function mpdata_diffuse_device_c(ncrms, nx, nz, ntracers, sl0, n, f, rho, adz, tkh, cx, cz, sb, st, zflux, &
        stream) bind(C, name=MPDATA_C_DIFFUSE_DEVICE)
      import :: c_int, c_int64_t, c_ptr
      integer(c_int64_t), value :: ncrms
      integer(c_int), value :: nx, nz, ntracers
      integer(c_int64_t), value :: sl0, n
      type(c_ptr), value :: f, rho, adz, tkh, cx, cz, sb, st, zflux
      type(c_ptr), value :: stream
    end function
    ! ---- large-scale vertical advection of f in place (include/mpdata_hip.h section 3m): cb, cc(n, nzm), dsum(n, nzm
    ! [, ntracers]) (c_null_ptr: skipped); device arrays of the plan's precision, asynchronous on the plan's stream;
    ! windowed plans are supported
    integer(c_int) function mpdata_plan_subside_device_c(plan, sl0, n, cb, cc, dsum, first_tracer, ntracers) &
        bind(C, name="mpdata_plan_subside_device")
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      type(c_ptr), value :: cb, cc, dsum
      integer(c_int), value :: first_tracer, ntracers
    end function
    ! ---- sedimentation of f in place (include/mpdata_hip.h section 3n): wp(n, nx, nzm [, ntracers]), psfc(n, nx
    ! [, ntracers]), pflux(n, nzm [, ntracers]) (c_null_ptr: skipped); device arrays of the plan's precision, asynchronous
    ! on the plan's stream; windowed plans are supported
    integer(c_int) function mpdata_plan_sediment_device_c(plan, sl0, n, wp, psfc, pflux, first_tracer, ntracers) &
        bind(C, name="mpdata_plan_sediment_device")
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      type(c_ptr), value :: wp, psfc, pflux
      integer(c_int), value :: first_tracer, ntracers
    end function
    ! ---- implicit vertical solve of f in place (include/mpdata_hip.h section 3o): lo, di, up(n, nzm), shared by the
    ! columns and the tracers; device arrays of the plan's precision, asynchronous on the plan's stream; windowed plans
    ! are supported
    integer(c_int) function mpdata_plan_vsolve_device_c(plan, sl0, n, lo, di, up, first_tracer, ntracers) &
        bind(C, name="mpdata_plan_vsolve_device")
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      type(c_ptr), value :: lo, di, up
      integer(c_int), value :: first_tracer, ntracers
    end function
    ! ---- implicit vertical diffusion of f with a per-cell diffusivity in place (include/mpdata_hip.h section 3s):
    ! tkh(n, 0:nx+1, nzm) and cz(n, nzm) as 3l takes them, sb, st(n, nx) (c_null_ptr: zero flux); device arrays of the
    ! plan's precision, asynchronous on the plan's stream; windowed plans are refused
    integer(c_int) function mpdata_plan_vdiffuse_device_c(plan, sl0, n, tkh, cz, sb, st, first_tracer, ntracers) &
        bind(C, name="mpdata_plan_vdiffuse_device")
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      type(c_ptr), value :: tkh, cz, sb, st
      integer(c_int), value :: first_tracer, ntracers
    end function
  end interface

  ! an interface block of its own for the bindings that take a REAL by value (the factor c below): the block above holds
  ! integers, handles and addresses only
  interface
    ! ---- per-cell sources of f in place (include/mpdata_hip.h section 3p): s(n, nx, nzm [, ntracers]), dsum(n, nzm
    ! [, ntracers]) (c_null_ptr: skipped); device arrays of the plan's precision, asynchronous on the plan's stream; c is a
    ! double for both precisions (rounded once to the plan's); mode MPDATA_CELL_ADD[_CLIP]; windowed plans are supported
    integer(c_int) function mpdata_plan_cell_add_device_c(plan, sl0, n, s, c, mode, dsum, first_tracer, ntracers) &
        bind(C, name="mpdata_plan_cell_add_device")
      import :: c_int, c_int64_t, c_ptr, c_double
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      type(c_ptr), value :: s
      real(c_double), value :: c
      integer(c_int), value :: mode
      type(c_ptr), value :: dsum
      integer(c_int), value :: first_tracer, ntracers
    end function
    ! ---- the fused column step of f in place (include/mpdata_hip.h section 3q): source (s, c, mode), subside (cb, cc),
    ! sediment (wp, psfc), vsolve (lo, di, up) in this order, a stage present exactly when its arrays are not c_null_ptr;
    ! s, wp(n, nx, nzm [, ntracers]), psfc(n, nx [, ntracers]), cb, cc, lo, di, up(n, nzm); device arrays of the plan's
    ! precision, asynchronous on the plan's stream; c is a double for both precisions; windowed plans are refused
    integer(c_int) function mpdata_plan_column_step_device_c(plan, sl0, n, s, c, mode, cb, cc, wp, psfc, lo, di, up, &
        first_tracer, ntracers) bind(C, name="mpdata_plan_column_step_device")
      import :: c_int, c_int64_t, c_ptr, c_double
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      type(c_ptr), value :: s
      real(c_double), value :: c
      integer(c_int), value :: mode
      type(c_ptr), value :: cb, cc, wp, psfc, lo, di, up
      integer(c_int), value :: first_tracer, ntracers
    end function
    ! ---- relaxation of f to a level profile in place (include/mpdata_hip.h section 3r): f = f - c * (f - m), m = target
    ! or, with target = c_null_ptr, the horizontal mean of f; c(n, nzm), target, mean(n, nzm [, ntracers]) (mean
    ! c_null_ptr: skipped); device arrays of the plan's precision, asynchronous on the plan's stream; windowed plans are
    ! supported
    integer(c_int) function mpdata_plan_relax_device_c(plan, sl0, n, c, target, mean, first_tracer, ntracers) &
        bind(C, name="mpdata_plan_relax_device")
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      type(c_ptr), value :: c, target, mean
      integer(c_int), value :: first_tracer, ntracers
    end function
    ! ---- first-order conversion from tracer src to tracer dst in place (include/mpdata_hip.h section 3t; tracers counted
    ! from 0): d = r * max(f_src - q0, 0), with mode MPDATA_CONVERT_LIMIT capped by max(f_src, 0); f_src = f_src - d,
    ! f_dst = f_dst + y * d; r, q0, y, dsum(n, nzm) (q0, y, dsum c_null_ptr: absent / skipped); device arrays of the plan's
    ! precision, asynchronous on the plan's stream; windowed plans are supported
    integer(c_int) function mpdata_plan_convert_device_c(plan, sl0, n, src, dst, r, q0, y, mode, dsum) &
        bind(C, name="mpdata_plan_convert_device")
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      integer(c_int), value :: src, dst
      type(c_ptr), value :: r, q0, y
      integer(c_int), value :: mode
      type(c_ptr), value :: dsum
    end function
    ! ---- per-level covariance of tracers ta and tb (include/mpdata_hip.h section 3u; tracers counted from 0; ta == tb: the
    ! variance): cov(n, nzm) = the SUM over the interior columns of (a - m_a) * (b - m_b), m = ma / mb(n, nzm) or
    ! (c_null_ptr) the horizontal mean of the row; mode MPDATA_LEVEL_COV_RAW: the sum of a * b, and ma, mb, mean_a, mean_b
    ! must be c_null_ptr; mean_a, mean_b(n, nzm) (c_null_ptr: skipped) take the means used; device arrays of the plan's
    ! precision, asynchronous on the plan's stream; nothing of the plan changes; windowed plans are supported
    integer(c_int) function mpdata_plan_level_cov_device_c(plan, sl0, n, ta, tb, ma, mb, mode, cov, mean_a, mean_b) &
        bind(C, name="mpdata_plan_level_cov_device")
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      integer(c_int), value :: ta, tb
      type(c_ptr), value :: ma, mb
      integer(c_int), value :: mode
      type(c_ptr), value :: cov, mean_a, mean_b
    end function
    ! ---- per-level conditional counts and sums (include/mpdata_hip.h section 3v; tracers counted from 0): a column is in
    ! where lo(n, nzm) < f(tc) <= hi(n, nzm) (c_null_ptr: that bound does not bind; one of the two is needed); cnt(n, nzm) =
    ! the number of interior columns that are in, csum(n, nzm, ntracers) = the SUM of tracers first_tracer .. first_tracer +
    ! ntracers - 1 over exactly those columns (c_null_ptr: skipped; one of the two is needed); device arrays of the plan's
    ! precision, asynchronous on the plan's stream; nothing of the plan changes; windowed plans are supported
    integer(c_int) function mpdata_plan_level_cond_device_c(plan, sl0, n, tc, lo, hi, cnt, csum, first_tracer, ntracers) &
        bind(C, name="mpdata_plan_level_cond_device")
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      integer(c_int), value :: tc
      type(c_ptr), value :: lo, hi, cnt, csum
      integer(c_int), value :: first_tracer, ntracers
    end function
    ! ---- per-column conditional level counts, tops and paths (include/mpdata_hip.h section 3w; tracers counted from 0): a
    ! level is in where lo(n, nzm) < f(tc) <= hi(n, nzm) (c_null_ptr: that bound does not bind; one of the two is needed;
    ! lo = +inf shuts a level out); kcnt(n, nx) = the levels of a column that are in, kbot, ktop(n, nx) = the lowest and the
    ! highest of them (0: none), cpath(n, nx, ntracers) = the sum of rho * adz * f of tracers first_tracer .. first_tracer +
    ! ntracers - 1 over exactly those levels, cover(n) = the columns with kcnt > 0 (needs kcnt), mass(n, ntracers) = the sum
    ! of cpath over the columns (needs cpath); c_null_ptr: skipped, one output is needed; device arrays of the plan's
    ! precision, asynchronous on the plan's stream; nothing of the plan changes; windowed plans are supported
    integer(c_int) function mpdata_plan_column_cond_device_c(plan, sl0, n, tc, lo, hi, kcnt, kbot, ktop, cpath, cover, mass, &
                                                             first_tracer, ntracers) &
        bind(C, name="mpdata_plan_column_cond_device")
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      integer(c_int), value :: tc
      type(c_ptr), value :: lo, hi, kcnt, kbot, ktop, cpath, cover, mass
      integer(c_int), value :: first_tracer, ntracers
    end function
    ! host arrays, all tracers (c_loc of real(c_double) arrays, or c_null_ptr), synchronous
    integer(c_int) function mpdata_plan_column_cond_c(plan, sl0, n, tc, lo, hi, kcnt, kbot, ktop, cpath, cover, mass) &
        bind(C, name="mpdata_plan_column_cond")
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      integer(c_int), value :: tc
      type(c_ptr), value :: lo, hi, kcnt, kbot, ktop, cpath, cover, mass
    end function
    ! ... of real(c_float) arrays, for fp32 plans
    integer(c_int) function mpdata_plan_column_cond_f32_c(plan, sl0, n, tc, lo, hi, kcnt, kbot, ktop, cpath, cover, mass) &
        bind(C, name="mpdata_plan_column_cond_f32")
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      integer(c_int), value :: tc
      type(c_ptr), value :: lo, hi, kcnt, kbot, ktop, cpath, cover, mass
    end function
    ! the same on instances [sl0, sl0 + n) of reference-layout device arrays f, rho(ncrms,nzm), adz(ncrms,nzm) of real(c_double)
    integer(c_int) function mpdata_column_cond_device_c(ncrms, nx, nz, ntracers, sl0, n, f, rho, adz, tc, lo, hi, kcnt, kbot, ktop, &
                                                        cpath, cover, mass, first_tracer, ntr, stream) &
        bind(C, name="mpdata_column_cond_device")
      import :: c_int, c_int64_t, c_ptr
      integer(c_int64_t), value :: ncrms
      integer(c_int), value :: nx, nz, ntracers
      integer(c_int64_t), value :: sl0, n
      type(c_ptr), value :: f, rho, adz
      integer(c_int), value :: tc
      type(c_ptr), value :: lo, hi, kcnt, kbot, ktop, cpath, cover, mass
      integer(c_int), value :: first_tracer, ntr
      type(c_ptr), value :: stream
    end function
    ! ... of real(c_float)
    integer(c_int) function mpdata_column_cond_f32_device_c(ncrms, nx, nz, ntracers, sl0, n, f, rho, adz, tc, lo, hi, kcnt, kbot, ktop, &
                                                        cpath, cover, mass, first_tracer, ntr, stream) &
        bind(C, name="mpdata_column_cond_f32_device")
      import :: c_int, c_int64_t, c_ptr
      integer(c_int64_t), value :: ncrms
      integer(c_int), value :: nx, nz, ntracers
      integer(c_int64_t), value :: sl0, n
      type(c_ptr), value :: f, rho, adz
      integer(c_int), value :: tc
      type(c_ptr), value :: lo, hi, kcnt, kbot, ktop, cpath, cover, mass
      integer(c_int), value :: first_tracer, ntr
      type(c_ptr), value :: stream
    end function
    ! ---- conservative per-level non-negativity fixer of f in place (include/mpdata_hip.h section 3x; tracers counted from
    ! 0): in every row (instance, level, tracer) with a negative interior cell the negative cells become +0 and the others
    ! are scaled by the row's sum over the sum of its positive cells, so that the row keeps its total (all +0 where the sum
    ! is not positive); a row without a negative cell keeps every bit; sum, nneg(n, nzm, ntracers) = the row sums of the old
    ! field and the negative cells of each row, written (c_null_ptr: skipped; both may be); device arrays of the plan's
    ! precision, asynchronous on the plan's stream; halo columns are neither read nor written; windowed plans are supported
    integer(c_int) function mpdata_plan_nonneg_device_c(plan, sl0, n, sum, nneg, first_tracer, ntracers) &
        bind(C, name="mpdata_plan_nonneg_device")
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      type(c_ptr), value :: sum, nneg
      integer(c_int), value :: first_tracer, ntracers
    end function
    ! host arrays, all tracers (c_loc of real(c_double) arrays, or c_null_ptr), synchronous
    integer(c_int) function mpdata_plan_nonneg_c(plan, sl0, n, sum, nneg) &
        bind(C, name="mpdata_plan_nonneg")
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      type(c_ptr), value :: sum, nneg
    end function
    ! ... of real(c_float) arrays, for fp32 plans
    integer(c_int) function mpdata_plan_nonneg_f32_c(plan, sl0, n, sum, nneg) &
        bind(C, name="mpdata_plan_nonneg_f32")
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      type(c_ptr), value :: sum, nneg
    end function
    ! the same on instances [sl0, sl0 + n) of a reference-layout device array f of real(c_double), in place
    integer(c_int) function mpdata_nonneg_device_c(ncrms, nx, nz, ntracers, sl0, n, f, sum, nneg, stream) &
        bind(C, name="mpdata_nonneg_device")
      import :: c_int, c_int64_t, c_ptr
      integer(c_int64_t), value :: ncrms
      integer(c_int), value :: nx, nz, ntracers
      integer(c_int64_t), value :: sl0, n
      type(c_ptr), value :: f, sum, nneg
      type(c_ptr), value :: stream
    end function
    ! ... of real(c_float)
    integer(c_int) function mpdata_nonneg_f32_device_c(ncrms, nx, nz, ntracers, sl0, n, f, sum, nneg, stream) &
        bind(C, name="mpdata_nonneg_f32_device")
      import :: c_int, c_int64_t, c_ptr
      integer(c_int64_t), value :: ncrms
      integer(c_int), value :: nx, nz, ntracers
      integer(c_int64_t), value :: sl0, n
      type(c_ptr), value :: f, sum, nneg
      type(c_ptr), value :: stream
    end function
    ! ---- saturation adjustment in place (include/mpdata_hip.h section 3y; tracers counted from 0): tracer tn becomes the
    ! condensate and, with tt >= 0, tracer tt the temperature diagnosed from the temperature-like tracer th and total water
    ! tq on the interior columns, by a Newton iteration per cell on the curves of par (c_loc of a type(mpdata_satadj_params));
    ! mode 0 or MPDATA_SATADJ_ICE; pres, gz, ncld, iters(n, nzm) (gz, ncld, iters c_null_ptr: absent / skipped); rows with
    ! pres == 0 keep every bit; device arrays of the plan's precision, asynchronous on the plan's stream; windowed plans are
    ! supported
    integer(c_int) function mpdata_plan_satadj_device_c(plan, sl0, n, th, tq, tn, tt, pres, gz, par, mode, ncld, iters) &
        bind(C, name="mpdata_plan_satadj_device")
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      integer(c_int), value :: th, tq, tn, tt
      type(c_ptr), value :: pres, gz, par
      integer(c_int), value :: mode
      type(c_ptr), value :: ncld, iters
    end function
    ! host arrays (c_loc of real(c_double) arrays, or c_null_ptr), synchronous
    integer(c_int) function mpdata_plan_satadj_c(plan, sl0, n, th, tq, tn, tt, pres, gz, par, mode, ncld, iters) &
        bind(C, name="mpdata_plan_satadj")
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      integer(c_int), value :: th, tq, tn, tt
      type(c_ptr), value :: pres, gz, par
      integer(c_int), value :: mode
      type(c_ptr), value :: ncld, iters
    end function
    ! ... of real(c_float) arrays, for fp32 plans
    integer(c_int) function mpdata_plan_satadj_f32_c(plan, sl0, n, th, tq, tn, tt, pres, gz, par, mode, ncld, iters) &
        bind(C, name="mpdata_plan_satadj_f32")
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      integer(c_int), value :: th, tq, tn, tt
      type(c_ptr), value :: pres, gz, par
      integer(c_int), value :: mode
      type(c_ptr), value :: ncld, iters
    end function
    ! the same on instances [sl0, sl0 + n) of a reference-layout device array f of real(c_double), in place
    integer(c_int) function mpdata_satadj_device_c(ncrms, nx, nz, ntracers, sl0, n, f, th, tq, tn, tt, pres, gz, par, mode, &
                                                   ncld, iters, stream) &
        bind(C, name="mpdata_satadj_device")
      import :: c_int, c_int64_t, c_ptr
      integer(c_int64_t), value :: ncrms
      integer(c_int), value :: nx, nz, ntracers
      integer(c_int64_t), value :: sl0, n
      type(c_ptr), value :: f
      integer(c_int), value :: th, tq, tn, tt
      type(c_ptr), value :: pres, gz, par
      integer(c_int), value :: mode
      type(c_ptr), value :: ncld, iters
      type(c_ptr), value :: stream
    end function
    ! ... of real(c_float)
    integer(c_int) function mpdata_satadj_f32_device_c(ncrms, nx, nz, ntracers, sl0, n, f, th, tq, tn, tt, pres, gz, par, mode, &
                                                       ncld, iters, stream) &
        bind(C, name="mpdata_satadj_f32_device")
      import :: c_int, c_int64_t, c_ptr
      integer(c_int64_t), value :: ncrms
      integer(c_int), value :: nx, nz, ntracers
      integer(c_int64_t), value :: sl0, n
      type(c_ptr), value :: f
      integer(c_int), value :: th, tq, tn, tt
      type(c_ptr), value :: pres, gz, par
      integer(c_int), value :: mode
      type(c_ptr), value :: ncld, iters
      type(c_ptr), value :: stream
    end function
    ! ---- linear combination of tracers in place (include/mpdata_hip.h section 3z; tracers counted from 0): on the interior
    ! columns f_dst = coef(:,:,1) * f_src(1) + coef(:,:,2) * f_src(2) + ... + c0, summed in the order of src, the sources read
    ! old also where one is dst; mode 0 or MPDATA_COMBINE_CLIP (v = v > 0 ? v : +0); src: c_loc of an integer(c_int) HOST
    ! array of nsrc <= MPDATA_COMBINE_MAX tracers (c_null_ptr with nsrc = 0, which needs c0); coef(n, nzm, nsrc), c0(n, nzm),
    ! sum(n, nzm) (each c_null_ptr: no multiply / nothing added / skipped); device arrays of the plan's precision,
    ! asynchronous on the plan's stream; windowed plans are supported
    ! (device arrays)
    integer(c_int) function mpdata_plan_combine_device_c(plan, sl0, n, dst, nsrc, src, coef, c0, mode, sum) &
        bind(C, name="mpdata_plan_combine_device")
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      integer(c_int), value :: dst, nsrc
      type(c_ptr), value :: src, coef, c0
      integer(c_int), value :: mode
      type(c_ptr), value :: sum
    end function
    ! host arrays (c_loc of real(c_double) arrays, or c_null_ptr), synchronous
    integer(c_int) function mpdata_plan_combine_c(plan, sl0, n, dst, nsrc, src, coef, c0, mode, sum) &
        bind(C, name="mpdata_plan_combine")
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      integer(c_int), value :: dst, nsrc
      type(c_ptr), value :: src, coef, c0
      integer(c_int), value :: mode
      type(c_ptr), value :: sum
    end function
    ! ... of real(c_float) arrays, for fp32 plans
    integer(c_int) function mpdata_plan_combine_f32_c(plan, sl0, n, dst, nsrc, src, coef, c0, mode, sum) &
        bind(C, name="mpdata_plan_combine_f32")
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      integer(c_int), value :: dst, nsrc
      type(c_ptr), value :: src, coef, c0
      integer(c_int), value :: mode
      type(c_ptr), value :: sum
    end function
    ! the same on instances [sl0, sl0 + n) of a reference-layout device array f of real(c_double), in place
    integer(c_int) function mpdata_combine_device_c(ncrms, nx, nz, ntracers, sl0, n, f, dst, nsrc, src, coef, c0, mode, sum, stream) &
        bind(C, name="mpdata_combine_device")
      import :: c_int, c_int64_t, c_ptr
      integer(c_int64_t), value :: ncrms
      integer(c_int), value :: nx, nz, ntracers
      integer(c_int64_t), value :: sl0, n
      type(c_ptr), value :: f
      integer(c_int), value :: dst, nsrc
      type(c_ptr), value :: src, coef, c0
      integer(c_int), value :: mode
      type(c_ptr), value :: sum
      type(c_ptr), value :: stream
    end function
    ! ... of real(c_float)
    integer(c_int) function mpdata_combine_f32_device_c(ncrms, nx, nz, ntracers, sl0, n, f, dst, nsrc, src, coef, c0, mode, sum, stream) &
        bind(C, name="mpdata_combine_f32_device")
      import :: c_int, c_int64_t, c_ptr
      integer(c_int64_t), value :: ncrms
      integer(c_int), value :: nx, nz, ntracers
      integer(c_int64_t), value :: sl0, n
      type(c_ptr), value :: f
      integer(c_int), value :: dst, nsrc
      type(c_ptr), value :: src, coef, c0
      integer(c_int), value :: mode
      type(c_ptr), value :: sum
      type(c_ptr), value :: stream
    end function
    ! ---- running column integral of tracer src into tracer dst, in place (include/mpdata_hip.h section 3aa; tracers counted
    ! from 0): on the interior columns p(k) = wgt(k) * f(k, src), s summed from the surface upward (mode
    ! MPDATA_COLUMN_SCAN_DOWN: from the top downward), f(k, dst) = s with p(k) (MPDATA_COLUMN_SCAN_EXCLUSIVE: without it),
    ! total = the final s; wgt(n, nzm) (c_null_ptr: rho * adz of the plan), total(n, nx) (c_null_ptr: skipped); device arrays
    ! of the plan's precision, asynchronous on the plan's stream; windowed plans are supported
    ! (device arrays)
    integer(c_int) function mpdata_plan_column_scan_device_c(plan, sl0, n, src, dst, wgt, total, mode) &
        bind(C, name="mpdata_plan_column_scan_device")
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      integer(c_int), value :: src, dst
      type(c_ptr), value :: wgt, total
      integer(c_int), value :: mode
    end function
    ! host arrays (c_loc of real(c_double) arrays, or c_null_ptr), synchronous
    integer(c_int) function mpdata_plan_column_scan_c(plan, sl0, n, src, dst, wgt, total, mode) &
        bind(C, name="mpdata_plan_column_scan")
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      integer(c_int), value :: src, dst
      type(c_ptr), value :: wgt, total
      integer(c_int), value :: mode
    end function
    ! ... of real(c_float) arrays, for fp32 plans
    integer(c_int) function mpdata_plan_column_scan_f32_c(plan, sl0, n, src, dst, wgt, total, mode) &
        bind(C, name="mpdata_plan_column_scan_f32")
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      integer(c_int), value :: src, dst
      type(c_ptr), value :: wgt, total
      integer(c_int), value :: mode
    end function
    ! the same on instances [sl0, sl0 + n) of a reference-layout device array f of real(c_double), in place; wgt is required
    integer(c_int) function mpdata_column_scan_device_c(ncrms, nx, nz, ntracers, sl0, n, f, src, dst, wgt, total, mode, stream) &
        bind(C, name="mpdata_column_scan_device")
      import :: c_int, c_int64_t, c_ptr
      integer(c_int64_t), value :: ncrms
      integer(c_int), value :: nx, nz, ntracers
      integer(c_int64_t), value :: sl0, n
      type(c_ptr), value :: f
      integer(c_int), value :: src, dst
      type(c_ptr), value :: wgt, total
      integer(c_int), value :: mode
      type(c_ptr), value :: stream
    end function
    ! ... of real(c_float)
    integer(c_int) function mpdata_column_scan_f32_device_c(ncrms, nx, nz, ntracers, sl0, n, f, src, dst, wgt, total, mode, stream) &
        bind(C, name="mpdata_column_scan_f32_device")
      import :: c_int, c_int64_t, c_ptr
      integer(c_int64_t), value :: ncrms
      integer(c_int), value :: nx, nz, ntracers
      integer(c_int64_t), value :: sl0, n
      type(c_ptr), value :: f
      integer(c_int), value :: src, dst
      type(c_ptr), value :: wgt, total
      integer(c_int), value :: mode
      type(c_ptr), value :: stream
    end function
    ! ---- per-level histograms (include/mpdata_hip.h section 3ab; tracers counted from 0): column i of a level is in bin j
    ! where edges(j) < f(tc) <= edges(j + 1), edges a HOST array of nb + 1 non-decreasing real(c_double) (c_loc of it) in
    ! every form; cnt(n, nzm, nb) = the number of interior columns in each bin, bsum(n, nzm, nb, ntracers) = the SUM of
    ! tracers first_tracer .. first_tracer + ntracers - 1 over exactly those columns (c_null_ptr: skipped; one of the two is
    ! needed); nothing of the plan changes; windowed plans are supported
    ! (device arrays of the plan's precision, asynchronous on the plan's stream)
    integer(c_int) function mpdata_plan_level_hist_device_c(plan, sl0, n, tc, nb, edges, cnt, bsum, first_tracer, ntracers) &
        bind(C, name="mpdata_plan_level_hist_device")
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      integer(c_int), value :: tc, nb
      type(c_ptr), value :: edges, cnt, bsum
      integer(c_int), value :: first_tracer, ntracers
    end function
    ! host arrays (c_loc of real(c_double) arrays, or c_null_ptr), all tracers, synchronous
    integer(c_int) function mpdata_plan_level_hist_c(plan, sl0, n, tc, nb, edges, cnt, bsum) &
        bind(C, name="mpdata_plan_level_hist")
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      integer(c_int), value :: tc, nb
      type(c_ptr), value :: edges, cnt, bsum
    end function
    ! ... of real(c_float) arrays, for fp32 plans (edges stays real(c_double))
    integer(c_int) function mpdata_plan_level_hist_f32_c(plan, sl0, n, tc, nb, edges, cnt, bsum) &
        bind(C, name="mpdata_plan_level_hist_f32")
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      integer(c_int), value :: tc, nb
      type(c_ptr), value :: edges, cnt, bsum
    end function
    ! the same on instances [sl0, sl0 + n) of a reference-layout device array f of real(c_double), which is only read
    integer(c_int) function mpdata_level_hist_device_c(ncrms, nx, nz, ntracers, sl0, n, f, tc, nb, edges, cnt, bsum, first_tracer, &
                                                       ntr, stream) bind(C, name="mpdata_level_hist_device")
      import :: c_int, c_int64_t, c_ptr
      integer(c_int64_t), value :: ncrms
      integer(c_int), value :: nx, nz, ntracers
      integer(c_int64_t), value :: sl0, n
      type(c_ptr), value :: f
      integer(c_int), value :: tc, nb
      type(c_ptr), value :: edges, cnt, bsum
      integer(c_int), value :: first_tracer, ntr
      type(c_ptr), value :: stream
    end function
    ! ... of real(c_float)
    integer(c_int) function mpdata_level_hist_f32_device_c(ncrms, nx, nz, ntracers, sl0, n, f, tc, nb, edges, cnt, bsum, first_tracer, &
                                                           ntr, stream) bind(C, name="mpdata_level_hist_f32_device")
      import :: c_int, c_int64_t, c_ptr
      integer(c_int64_t), value :: ncrms
      integer(c_int), value :: nx, nz, ntracers
      integer(c_int64_t), value :: sl0, n
      type(c_ptr), value :: f
      integer(c_int), value :: tc, nb
      type(c_ptr), value :: edges, cnt, bsum
      integer(c_int), value :: first_tracer, ntr
      type(c_ptr), value :: stream
    end function
    ! ---- per-level updraft / downdraft sampling (include/mpdata_hip.h section 3ac; tracers counted from 0, tc = -1: no
    ! tracer condition): with wc = 0.5 * (w(k) + w(k+1)) (+0 above the top) a column of a level where lo < f(tc) <= hi is in
    ! class UP (0) where wc > wup, DOWN (1) where wc < wdn, ENV (2) otherwise; cnt(n, nzm, 3) = the columns of each class,
    ! wsum(n, nzm, 3) = the SUM of wc over them, fsum and wfsum(n, nzm, 3, ntracers) = the sums of tracers first_tracer ..
    ! first_tracer + ntracers - 1 and of wc times them (c_null_ptr: skipped; one of the four is needed; lo, hi: c_null_ptr
    ! does not bind); the plan must hold w; nothing of the plan changes; windowed plans are supported
    ! (device arrays of the plan's precision, asynchronous on the plan's stream)
    integer(c_int) function mpdata_plan_level_draft_device_c(plan, sl0, n, tc, lo, hi, wup, wdn, cnt, wsum, fsum, wfsum, &
                                                             first_tracer, ntracers) bind(C, name="mpdata_plan_level_draft_device")
      import :: c_int, c_int64_t, c_ptr, c_double
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      integer(c_int), value :: tc
      type(c_ptr), value :: lo, hi
      real(c_double), value :: wup, wdn
      type(c_ptr), value :: cnt, wsum, fsum, wfsum
      integer(c_int), value :: first_tracer, ntracers
    end function
    ! host arrays (c_loc of real(c_double) arrays, or c_null_ptr), all tracers, synchronous
    integer(c_int) function mpdata_plan_level_draft_c(plan, sl0, n, tc, lo, hi, wup, wdn, cnt, wsum, fsum, wfsum) &
        bind(C, name="mpdata_plan_level_draft")
      import :: c_int, c_int64_t, c_ptr, c_double
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      integer(c_int), value :: tc
      type(c_ptr), value :: lo, hi
      real(c_double), value :: wup, wdn
      type(c_ptr), value :: cnt, wsum, fsum, wfsum
    end function
    ! ... of real(c_float) arrays, for fp32 plans (wup, wdn stay real(c_double))
    integer(c_int) function mpdata_plan_level_draft_f32_c(plan, sl0, n, tc, lo, hi, wup, wdn, cnt, wsum, fsum, wfsum) &
        bind(C, name="mpdata_plan_level_draft_f32")
      import :: c_int, c_int64_t, c_ptr, c_double
      type(c_ptr), value :: plan
      integer(c_int64_t), value :: sl0, n
      integer(c_int), value :: tc
      type(c_ptr), value :: lo, hi
      real(c_double), value :: wup, wdn
      type(c_ptr), value :: cnt, wsum, fsum, wfsum
    end function
    ! the same on instances [sl0, sl0 + n) of reference-layout device arrays f and w of real(c_double), which are only read
    integer(c_int) function mpdata_level_draft_device_c(ncrms, nx, nz, ntracers, sl0, n, f, w, tc, lo, hi, wup, wdn, cnt, wsum, &
                                     fsum, wfsum, first_tracer, ntr, stream) bind(C, name="mpdata_level_draft_device")
      import :: c_int, c_int64_t, c_ptr, c_double
      integer(c_int64_t), value :: ncrms
      integer(c_int), value :: nx, nz, ntracers
      integer(c_int64_t), value :: sl0, n
      type(c_ptr), value :: f, w
      integer(c_int), value :: tc
      type(c_ptr), value :: lo, hi
      real(c_double), value :: wup, wdn
      type(c_ptr), value :: cnt, wsum, fsum, wfsum
      integer(c_int), value :: first_tracer, ntr
      type(c_ptr), value :: stream
    end function
    ! ... of real(c_float)
    integer(c_int) function mpdata_level_draft_f32_device_c(ncrms, nx, nz, ntracers, sl0, n, f, w, tc, lo, hi, wup, wdn, cnt, wsum, &
                                     fsum, wfsum, first_tracer, ntr, stream) bind(C, name="mpdata_level_draft_f32_device")
      import :: c_int, c_int64_t, c_ptr, c_double
      integer(c_int64_t), value :: ncrms
      integer(c_int), value :: nx, nz, ntracers
      integer(c_int64_t), value :: sl0, n
      type(c_ptr), value :: f, w
      integer(c_int), value :: tc
      type(c_ptr), value :: lo, hi
      real(c_double), value :: wup, wdn
      type(c_ptr), value :: cnt, wsum, fsum, wfsum
      integer(c_int), value :: first_tracer, ntr
      type(c_ptr), value :: stream
    end function
  end interface

  type(c_ptr), save :: resident_plan = c_null_ptr
  ! scatter / gather record of the last multi-GPU transfer (advect_transfer_stats)
  real(c_double), save :: last_scatter_s = 0, last_gather_s = 0
  integer(c_int64_t), save :: last_scatter_bytes = 0, last_gather_bytes = 0

contains

  !> `error stop` with the library's message when a C-ABI call failed
  !! (the reference has no error path at all; a failure there is a crash).
  subroutine mpdata_check(rc, what)
    integer(c_int), intent(in) :: rc
    character(*), intent(in) :: what
    character(kind=c_char), pointer :: msg(:)
    integer :: n
    if (rc == 0) return
    call c_f_pointer(mpdata_last_error_c(), msg, [512])
    n = 1
    do while (n < 512 .and. msg(n) /= c_null_char)
      n = n + 1
    end do
    write(*,*) 'libmpdata_hip: ', what, ' failed, rc=', rc, ': ', msg(1:n-1)
    error stop 1
  end subroutine mpdata_check

  !> Outflow Courant number of the velocities a resident plan holds (include/mpdata_hip.h section 3h), whole plan:
  !! clev(nslices, nzm) and cinst(nslices) are DEVICE addresses (c_null_ptr: skipped, not both); asynchronous on the
  !! plan's stream.  A step is stable for the upwind pass where cinst <= 1; what SAM asks `kurant` for.
  subroutine mpdata_plan_courant_device(plan, clev, cinst)
    type(c_ptr), intent(in) :: plan, clev, cinst
    call mpdata_check(mpdata_plan_courant_device_c(plan, 0_c_int64_t, nslices, clev, cinst), 'mpdata_plan_courant_device')
  end subroutine mpdata_plan_courant_device

  !> Drop-in replacement of `call advect_scalar2D_openacc_N(f,u,w,rho,rhow,flux)`
  !! (reference :53, :57): synchronous, host arrays, transfers included (the
  !! reference's `!$acc update device/host`, :107 and :241).
  subroutine advect_scalar2D(f, u, w, rho, rhow, flux)
    real(rp), intent(inout) :: f    (nslices, -2:nx+3, 1, nzm, ntracers)
    real(rp), intent(in   ) :: u    (nslices, -1:nx+3, 1, nzm)
    real(rp), intent(in   ) :: w    (nslices, -1:nx+2, 1, nz )
    real(rp), intent(in   ) :: rho  (nslices, nzm)
    real(rp), intent(in   ) :: rhow (nslices, nz )
    real(rp), intent(inout) :: flux (nslices, nz, ntracers)   ! level nz is left as it came (reference :541,:624)
    type(c_ptr) :: plan
    if (ngpus <= 1) then
      call mpdata_check(mpdata_advect_scalar2d_c(nslices, nx, nz, ntracers, f, u, w, rho, rhow, adz, flux), &
                        'mpdata_advect_scalar2d')
    else
      ! ncrms sharded over `ngpus` GPUs: scatter (RCCL over xGMI), one kernel per GPU, gather
      call create_plan(plan)
      call mpdata_check(mpdata_plan_upload_c(plan, f, u, w, rho, rhow, adz, flux), 'mpdata_plan_upload')
      call mpdata_check(mpdata_plan_run_c(plan), 'mpdata_plan_run')
      call mpdata_check(mpdata_plan_sync_c(plan), 'mpdata_plan_sync')
      call mpdata_check(mpdata_plan_download_c(plan, f, flux), 'mpdata_plan_download')
      call record_stats(plan)
      call mpdata_check(mpdata_plan_destroy_c(plan), 'mpdata_plan_destroy')
    end if
  end subroutine advect_scalar2D

  subroutine create_plan(plan)
    type(c_ptr), intent(out) :: plan
    if (ngpus <= 1) then
      call mpdata_check(mpdata_plan_create_c(nslices, nx, nz, ntracers, plan), 'mpdata_plan_create')
    else
#ifdef MPDATA_SINGLE
      write(*,*) 'multi-GPU plans are fp64'
      error stop 1
#else
      call mpdata_check(mpdata_plan_create_multi_c(nslices, nx, nz, ntracers, ngpus, plan), 'mpdata_plan_create_multi')
#endif
    end if
  end subroutine create_plan

  subroutine record_stats(plan)
    type(c_ptr), intent(in) :: plan
    integer(c_int) :: tr
    if (ngpus <= 1) return
    call mpdata_check(mpdata_plan_transfer_stats_c(plan, last_scatter_s, last_gather_s, last_scatter_bytes, &
                                                   last_gather_bytes, tr), 'mpdata_plan_transfer_stats')
  end subroutine record_stats

  !> seconds and bytes per peer link of the last multi-GPU scatter (upload) / gather (download)
  subroutine advect_transfer_stats(scatter_s, gather_s, scatter_bytes, gather_bytes)
    real(c_double), intent(out) :: scatter_s, gather_s
    integer(c_int64_t), intent(out) :: scatter_bytes, gather_bytes
    scatter_s = last_scatter_s; gather_s = last_gather_s
    scatter_bytes = last_scatter_bytes; gather_bytes = last_gather_bytes
  end subroutine advect_transfer_stats

  !> The whole sequence with the GLOBAL arrays resident on the root GPU instead of the host: the
  !! inputs are generated there (mpdata_fill_synthetic_device: the law init() uses, element for
  !! element), handed to the plan by mpdata_plan_import_device -- for ngpus > 1 that is the scatter
  !! over RCCL / xGMI, the replacement of the reference's `update device` (:107) --, advected (the
  !! reference's timed region, :110-:238), gathered back (`update host`, :241) and summed on the
  !! device.  No host array of the problem's size exists: BASELINE.json configs[4] (ncrms = 524288 x
  !! 25 tracers: 107.6 GB of f) runs from a host with a few GB.  fp64 only.
  subroutine advect_device_problem_run(seed, dist, kernel_ms, wall_s, sum_f, sum_flux, ranks)
    integer(c_int64_t), intent(in) :: seed
    integer, intent(in) :: dist
    real(c_double), intent(out) :: kernel_ms, wall_s, sum_f, sum_flux
    integer, intent(out) :: ranks
#ifdef MPDATA_SINGLE
    write(*,*) 'the device-resident mode is fp64'
    error stop 1
#else
    type(c_ptr) :: plan, d(0:6)
    integer(c_int64_t) :: rows(0:6), n, nf, nx1
    integer(8) :: t1, t2, tr
    integer :: i
    ! generator ids (the reference's fill order, :654-660): 0 adz, 1 f, 2 u, 3 w, 4 rho, 5 rhow, 6 flux
    rows = [ int(nzm, 8), int(nx+6, 8)*nzm*ntracers, int(nx+5, 8)*nzm, int(nx+4, 8)*nz, int(nzm, 8), int(nz, 8), &
             int(nz, 8)*ntracers ]
    ! the plan first: the global arrays must live on ITS root GPU (shard 0's device; with
    ! MPDATA_MULTI_DEVICES=3,4 that is device 3, not the current one)
    call create_plan(plan)
    do i = 0, 6
      call mpdata_check(mpdata_plan_device_alloc_c(plan, d(i), rows(i)*nslices*8_8), 'mpdata_plan_device_alloc')
      call mpdata_check(mpdata_fill_synthetic_device_c(d(i), int(i, c_int), rows(i), nslices, 0_8, nslices, seed, &
                                                       int(dist, c_int), c_null_ptr), 'mpdata_fill_synthetic_device')
    end do
    ranks = mpdata_plan_ranks_seen_c(plan)
    ! scatter (ngpus > 1) / layout entry; twice: the first run is the warm-up the reference's first
    ! OpenACC call pays as well, the second import restores the inputs for the timed run
    do i = 1, 2
      call mpdata_check(mpdata_plan_import_device_c(plan, d(1), d(2), d(3), d(4), d(5), d(0), d(6), 0_c_int, &
                                                    int(ntracers, c_int)), 'mpdata_plan_import_device')
      call mpdata_check(mpdata_plan_sync_c(plan), 'mpdata_plan_sync')
      call system_clock(t1)
      call mpdata_check(mpdata_plan_run_c(plan), 'mpdata_plan_run')
      call mpdata_check(mpdata_plan_sync_c(plan), 'mpdata_plan_sync')
      call system_clock(t2, tr)
    end do
    wall_s = dble(t2-t1)/dble(tr)
    call mpdata_check(mpdata_plan_last_kernel_ms_c(plan, kernel_ms), 'mpdata_plan_last_kernel_ms')
    call mpdata_check(mpdata_plan_export_device_c(plan, d(1), d(6), 0_c_int, int(ntracers, c_int)), 'mpdata_plan_export_device')
    call mpdata_check(mpdata_plan_sync_c(plan), 'mpdata_plan_sync')
    call record_stats(plan)
    nf = rows(1)*nslices
    call mpdata_check(mpdata_device_sum_c(d(1), nf, nf, nf, sum_f), 'mpdata_device_sum')
    n = rows(6)*nslices; nx1 = int(nz, 8)*nslices     ! flux(:,1:nzm,:) -- level nz is never written (:541, :624)
    call mpdata_check(mpdata_device_sum_c(d(6), n, int(nzm, 8)*nslices, nx1, sum_flux), 'mpdata_device_sum')
    call mpdata_check(mpdata_plan_destroy_c(plan), 'mpdata_plan_destroy')
    do i = 0, 6
      call mpdata_check(mpdata_device_free_c(d(i)), 'mpdata_device_free')
    end do
#endif
  end subroutine advect_device_problem_run

  !> Device-resident form = the reference's timed region (:105-110, :237-242):
  !! begin = `enter data` + `update device`; run = the kernels + `wait`;
  !! end = `update host`.
  subroutine advect_resident_begin(f, u, w, rho, rhow, flux)
    real(rp), intent(in) :: f(nslices, -2:nx+3, 1, nzm, ntracers), u(nslices, -1:nx+3, 1, nzm), w(nslices, -1:nx+2, 1, nz)
    real(rp), intent(in) :: rho(nslices, nzm), rhow(nslices, nz), flux(nslices, nz, ntracers)
    call create_plan(resident_plan)
    call mpdata_check(mpdata_plan_upload_c(resident_plan, f, u, w, rho, rhow, adz, flux), 'mpdata_plan_upload')
  end subroutine advect_resident_begin

  subroutine advect_resident_run(kernel_ms)
    real(rp), intent(out), optional :: kernel_ms
    real(c_double) :: ms
    call mpdata_check(mpdata_plan_run_c(resident_plan), 'mpdata_plan_run')
    call mpdata_check(mpdata_plan_sync_c(resident_plan), 'mpdata_plan_sync')
    if (present(kernel_ms)) then
      call mpdata_check(mpdata_plan_last_kernel_ms_c(resident_plan, ms), 'mpdata_plan_last_kernel_ms')
      kernel_ms = real(ms, rp)
    end if
  end subroutine advect_resident_run

  subroutine advect_resident_end(f, flux)
    real(rp), intent(out) :: f(nslices, -2:nx+3, 1, nzm, ntracers)
    real(rp), intent(inout) :: flux(nslices, nz, ntracers)
    call mpdata_check(mpdata_plan_download_c(resident_plan, f, flux), 'mpdata_plan_download')
    call record_stats(resident_plan)
    call mpdata_check(mpdata_plan_destroy_c(resident_plan), 'mpdata_plan_destroy')
    resident_plan = c_null_ptr
  end subroutine advect_resident_end

end module mpdata_hip_mod
