! column_cond_calls.F90 -- a TEST program: the per-column conditional level counts, tops and paths of a resident plan's
! tracers (include/mpdata_hip.h section 3w) driven from Fortran through the interfaces of mpdata_hip_mod alone.  It has no
! oracle and no interface block of its own for a library name.
!
!   ./column_cond_calls <input file> <dump file>       (column_cond_calls_sp: the -DMPDATA_SINGLE build, rp = c_float)
!
! Both files are streams of records in the format of calls_common.F90, which holds the helpers and the frame around the
! calls below as well (calls_open, calls_import, calls_close).  The input file is written by tests/test_plan_column_cond.py,
! which replays the script on the numpy model and compares every record of the dump bit for bit, the return code of every
! call included: a code is recorded, never stopped on.  Of `params`, t1 is the condition tracer of the first and the third
! call and tn that of the second.
!
! The script: create, set_boundary(PERIODIC), import_device of all seven arrays - the device form on the block (sl0, n),
! tracer t1 inside (lo_a, hi_a], all six outputs of all T tracers - the host form on the whole plan, tracer tn above lo_b,
! kcnt and cover alone - the array form on the block of the device arrays the plan was filled from, tracer t1 up to hi_c,
! cpath and mass of tracer tn alone - a call without a bound, which is refused - run - export_device (the calls changed
! nothing) - destroy.
! The host form and the array form of the program's precision: the module binds both precisions by their literal names.
#ifdef MPDATA_SINGLE
#define COLUMN_COND_HOST mpdata_plan_column_cond_f32_c
#define COLUMN_COND_ARRAY mpdata_column_cond_f32_device_c
#else
#define COLUMN_COND_HOST mpdata_plan_column_cond_c
#define COLUMN_COND_ARRAY mpdata_column_cond_device_c
#endif
program column_cond_calls
  use iso_c_binding
  use mpdata_grid
  use mpdata_hip_mod
  use calls_common
  implicit none
  real(rp), allocatable, target :: lo_a(:,:), hi_a(:,:), lo_b(:,:), hi_c(:,:)
  real(rp), allocatable, target :: kcnt_a(:,:), kbot_a(:,:), ktop_a(:,:), cpath_a(:,:,:), cover_a(:), mass_a(:,:)
  real(rp), allocatable, target :: kcnt_b(:,:), cover_b(:), cpath_c(:,:), mass_c(:)
  type(c_ptr) :: d_lo, d_hi, d_kcnt, d_kbot, d_ktop, d_cpath, d_cover, d_mass

  call calls_open('column_cond_calls')
  allocate(lo_a(n, nzm), hi_a(n, nzm), lo_b(ncrms, nzm), hi_c(n, nzm))
  allocate(kcnt_a(n, nx), kbot_a(n, nx), ktop_a(n, nx), cpath_a(n, nx, T), cover_a(n), mass_a(n, T))
  allocate(kcnt_b(ncrms, nx), cover_b(ncrms), cpath_c(n, nx), mass_c(n))
  call get_r('lo_a', lo_a, shape(lo_a)); call get_r('hi_a', hi_a, shape(hi_a))
  call get_r('lo_b', lo_b, shape(lo_b)); call get_r('hi_c', hi_c, shape(hi_c))
  call dalloc(d_lo, size(lo_a)); call dalloc(d_hi, size(hi_a))
  call dalloc(d_kcnt, size(kcnt_a)); call dalloc(d_kbot, size(kbot_a)); call dalloc(d_ktop, size(ktop_a))
  call dalloc(d_cpath, size(cpath_a)); call dalloc(d_cover, size(cover_a)); call dalloc(d_mass, size(mass_a))
  call calls_import()

  ! ---- the device form: the block, t1 inside (lo, hi], every output, all tracers
  kcnt_a = SENTINEL; kbot_a = SENTINEL; ktop_a = SENTINEL; cpath_a = SENTINEL; cover_a = SENTINEL; mass_a = SENTINEL
  call to_dev(d_lo, lo_a, size(lo_a)); call to_dev(d_hi, hi_a, size(hi_a))
  call to_dev(d_kcnt, kcnt_a, size(kcnt_a)); call to_dev(d_kbot, kbot_a, size(kbot_a)); call to_dev(d_ktop, ktop_a, size(ktop_a))
  call to_dev(d_cpath, cpath_a, size(cpath_a)); call to_dev(d_cover, cover_a, size(cover_a)); call to_dev(d_mass, mass_a, size(mass_a))
  call note(mpdata_plan_column_cond_device_c(plan, sl0, n, int(t1, c_int), d_lo, d_hi, d_kcnt, d_kbot, d_ktop, d_cpath, d_cover, &
                                             d_mass, 0_c_int, int(T, c_int)), 'cond_block')
  call note(mpdata_plan_sync_c(plan), 'sync')
  call to_host(kcnt_a, d_kcnt, size(kcnt_a)); call put_r('kcnt_a', kcnt_a, shape(kcnt_a))
  call to_host(kbot_a, d_kbot, size(kbot_a)); call put_r('kbot_a', kbot_a, shape(kbot_a))
  call to_host(ktop_a, d_ktop, size(ktop_a)); call put_r('ktop_a', ktop_a, shape(ktop_a))
  call to_host(cpath_a, d_cpath, size(cpath_a)); call put_r('cpath_a', cpath_a, shape(cpath_a))
  call to_host(cover_a, d_cover, size(cover_a)); call put_r('cover_a', cover_a, shape(cover_a))
  call to_host(mass_a, d_mass, size(mass_a)); call put_r('mass_a', mass_a, shape(mass_a))

  ! ---- the host form: the whole plan, tn above lo, the count and the cover alone
  kcnt_b = SENTINEL; cover_b = SENTINEL
  call note(COLUMN_COND_HOST(plan, 0_c_int64_t, ncrms, int(tn, c_int), c_loc(lo_b), c_null_ptr, c_loc(kcnt_b), c_null_ptr, &
                             c_null_ptr, c_null_ptr, c_loc(cover_b), c_null_ptr), 'cond_host')
  call put_r('kcnt_b', kcnt_b, shape(kcnt_b)); call put_r('cover_b', cover_b, shape(cover_b))

  ! ---- the array form: the block of the arrays the plan was filled from, t1 up to hi, the path and the mass of tracer tn
  cpath_c = SENTINEL; mass_c = SENTINEL
  call to_dev(d_hi, hi_c, size(hi_c)); call to_dev(d_cpath, cpath_c, size(cpath_c)); call to_dev(d_mass, mass_c, size(mass_c))
  call note(COLUMN_COND_ARRAY(ncrms, nx, nz, int(T, c_int), sl0, n, d_f, d_rho, d_adz, int(t1, c_int), c_null_ptr, d_hi, &
                              c_null_ptr, c_null_ptr, c_null_ptr, d_cpath, c_null_ptr, d_mass, int(tn, c_int), 1_c_int, &
                              c_null_ptr), 'cond_array')
  call note(hipDeviceSynchronize(), 'dsync')
  call to_host(cpath_c, d_cpath, size(cpath_c)); call put_r('cpath_c', cpath_c, shape(cpath_c))
  call to_host(mass_c, d_mass, size(mass_c)); call put_r('mass_c', mass_c, shape(mass_c))

  ! ---- refused: no bound at all
  call note(mpdata_plan_column_cond_device_c(plan, 0_c_int64_t, ncrms, int(t1, c_int), c_null_ptr, c_null_ptr, d_kcnt, c_null_ptr, &
                                             c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, 0_c_int, int(T, c_int)), 'cond_refused')

  call calls_close()
  call dfree(d_lo); call dfree(d_hi); call dfree(d_kcnt); call dfree(d_kbot); call dfree(d_ktop)
  call dfree(d_cpath); call dfree(d_cover); call dfree(d_mass)
end program column_cond_calls
