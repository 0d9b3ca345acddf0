! level_cov_calls.F90 -- a TEST program: the per-level covariance of two tracers of a resident plan (include/mpdata_hip.h
! section 3u) driven from Fortran through the interfaces of mpdata_hip_mod alone.  It has no oracle and no interface block
! of its own for a library name.
!
!   ./level_cov_calls <input file> <dump file>       (level_cov_calls_sp: the -DMPDATA_SINGLE build, rp = c_float)
!
! Both files are streams of records in the format of calls_common.F90, which holds the helpers and the frame around the
! calls below as well (calls_open, calls_import, calls_close).  The input file is written by tests/test_plan_level_cov.py,
! which replays the script on the numpy model and compares every record of the dump bit for bit, the return code of every
! call included: a code is recorded, never stopped on.  Of `params`, t1 is the tracer ta and tn the tracer tb here.
!
! The script: create, set_boundary(PERIODIC), import_device of all seven arrays - the covariance of (ta, tb) on the block
! (sl0, n), both means formed and returned - (tb, ta) on the whole plan about the given profile ma, the other mean formed
! and returned - the RAW second moment of ta with itself on the whole plan - a RAW call with a profile, which is refused -
! run - export_device (the call changed nothing) - destroy.
program level_cov_calls
  use iso_c_binding
  use mpdata_grid
  use mpdata_hip_mod
  use calls_common
  implicit none
  real(rp), allocatable, target :: ma_b(:,:), cov_a(:,:), mean_a_a(:,:), mean_b_a(:,:), cov_b(:,:), mean_b_b(:,:), cov_c(:,:)
  type(c_ptr) :: d_ma, d_cov, d_mean_a, d_mean_b

  call calls_open('level_cov_calls')
  allocate(ma_b(ncrms, nzm), cov_a(n, nzm), mean_a_a(n, nzm), mean_b_a(n, nzm), cov_b(ncrms, nzm), mean_b_b(ncrms, nzm), &
           cov_c(ncrms, nzm))
  call get_r('ma_b', ma_b, shape(ma_b))
  call dalloc(d_ma, size(ma_b)); call dalloc(d_cov, size(cov_b)); call dalloc(d_mean_a, size(cov_b))
  call dalloc(d_mean_b, size(cov_b))
  call calls_import()

  ! ---- the block, (ta, tb), both means formed and returned
  cov_a = SENTINEL; mean_a_a = SENTINEL; mean_b_a = SENTINEL
  call to_dev(d_cov, cov_a, size(cov_a)); call to_dev(d_mean_a, mean_a_a, size(mean_a_a))
  call to_dev(d_mean_b, mean_b_a, size(mean_b_a))
  call note(mpdata_plan_level_cov_device_c(plan, sl0, n, int(t1, c_int), int(tn, c_int), c_null_ptr, c_null_ptr, 0_c_int, &
                                           d_cov, d_mean_a, d_mean_b), 'cov_block')
  call note(mpdata_plan_sync_c(plan), 'sync')
  call to_host(cov_a, d_cov, size(cov_a)); call put_r('cov_a', cov_a, shape(cov_a))
  call to_host(mean_a_a, d_mean_a, size(mean_a_a)); call put_r('mean_a_a', mean_a_a, shape(mean_a_a))
  call to_host(mean_b_a, d_mean_b, size(mean_b_a)); call put_r('mean_b_a', mean_b_a, shape(mean_b_a))

  ! ---- the whole plan, (tb, ta), about the given ma; the mean of the second tracer formed and returned
  cov_b = SENTINEL; mean_b_b = SENTINEL
  call to_dev(d_ma, ma_b, size(ma_b)); call to_dev(d_cov, cov_b, size(cov_b)); call to_dev(d_mean_b, mean_b_b, size(mean_b_b))
  call note(mpdata_plan_level_cov_device_c(plan, 0_c_int64_t, ncrms, int(tn, c_int), int(t1, c_int), d_ma, c_null_ptr, 0_c_int, &
                                           d_cov, c_null_ptr, d_mean_b), 'cov_given')
  call note(mpdata_plan_sync_c(plan), 'sync')
  call to_host(cov_b, d_cov, size(cov_b)); call put_r('cov_b', cov_b, shape(cov_b))
  call to_host(mean_b_b, d_mean_b, size(mean_b_b)); call put_r('mean_b_b', mean_b_b, shape(mean_b_b))

  ! ---- the whole plan, the RAW second moment of ta
  cov_c = SENTINEL
  call to_dev(d_cov, cov_c, size(cov_c))
  call note(mpdata_plan_level_cov_device_c(plan, 0_c_int64_t, ncrms, int(t1, c_int), int(t1, c_int), c_null_ptr, c_null_ptr, &
                                           MPDATA_LEVEL_COV_RAW, d_cov, c_null_ptr, c_null_ptr), 'cov_raw')
  call note(mpdata_plan_sync_c(plan), 'sync')
  call to_host(cov_c, d_cov, size(cov_c)); call put_r('cov_c', cov_c, shape(cov_c))

  ! ---- refused: RAW subtracts no mean, so it takes no profile
  call note(mpdata_plan_level_cov_device_c(plan, 0_c_int64_t, ncrms, int(t1, c_int), int(tn, c_int), d_ma, c_null_ptr, &
                                           MPDATA_LEVEL_COV_RAW, d_cov, c_null_ptr, c_null_ptr), 'cov_refused')

  call calls_close()
  call dfree(d_ma); call dfree(d_cov); call dfree(d_mean_a); call dfree(d_mean_b)
end program level_cov_calls
