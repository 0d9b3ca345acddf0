! column_scan_calls.F90 -- a TEST program: running column integrals of the tracers of a resident plan (include/mpdata_hip.h
! section 3aa) driven from Fortran through the interfaces of mpdata_hip_mod alone.  It has no oracle and no interface block
! of its own for a library name.
!
!   ./column_scan_calls <input file> <dump file>       (column_scan_calls_sp: the -DMPDATA_SINGLE build, rp = c_float)
!
! Both files are streams of records in the format of calls_common.F90, which holds the helpers and the frame around the
! calls below as well (calls_open, calls_import, calls_close).  The input file is written by
! tests/test_plan_column_scan.py, which replays the script on the numpy model and compares every record of the dump bit for
! bit, the return code of every call included: a code is recorded, never stopped on.  Of `params`, t1 is the source tracer
! and tn the tracer dst here.
!
! The script: create, set_boundary(PERIODIC), import_device of all seven arrays - the scan of t1 into dst on the block
! (sl0, n), upward and inclusive, with wgt and total - the scan of dst in place on the whole plan, downward and exclusive,
! with rho * adz of the plan (no wgt) and total - the HOST form on the block: dst into t1, downward, with wgt and total - a
! call with an unknown mode bit, which is refused - run - export_device - destroy.
program column_scan_calls
  use iso_c_binding
  use mpdata_grid
  use mpdata_hip_mod
  use calls_common
  implicit none
  real(rp), allocatable, target :: wgt_a(:,:), wgt_c(:,:), total_a(:,:), total_b(:,:), total_c(:,:)
  type(c_ptr) :: d_wgt, d_total

  call calls_open('column_scan_calls')
  allocate(wgt_a(n, nzm), wgt_c(n, nzm), total_a(n, nx), total_b(ncrms, nx), total_c(n, nx))
  call get_r('wgt_a', wgt_a, shape(wgt_a)); call get_r('wgt_c', wgt_c, shape(wgt_c))
  call dalloc(d_wgt, size(wgt_a)); call dalloc(d_total, size(total_b))
  call calls_import()

  ! ---- the block: t1 into dst, upward, inclusive, with wgt and total
  total_a = SENTINEL
  call to_dev(d_wgt, wgt_a, size(wgt_a)); call to_dev(d_total, total_a, size(total_a))
  call note(mpdata_plan_column_scan_device_c(plan, sl0, n, int(t1, c_int), int(tn, c_int), d_wgt, d_total, 0_c_int), 'scan_block')
  call note(mpdata_plan_sync_c(plan), 'sync')
  call to_host(total_a, d_total, size(total_a)); call put_r('total_a', total_a, shape(total_a))

  ! ---- the whole plan: dst in place, downward, exclusive, rho * adz of the plan
  total_b = SENTINEL
  call to_dev(d_total, total_b, size(total_b))
  call note(mpdata_plan_column_scan_device_c(plan, 0_c_int64_t, ncrms, int(tn, c_int), int(tn, c_int), c_null_ptr, d_total, &
                                             ior(MPDATA_COLUMN_SCAN_DOWN, MPDATA_COLUMN_SCAN_EXCLUSIVE)), 'scan_dn_excl')
  call note(mpdata_plan_sync_c(plan), 'sync')
  call to_host(total_b, d_total, size(total_b)); call put_r('total_b', total_b, shape(total_b))

  ! ---- the host form on the block: dst into t1, downward
  total_c = SENTINEL
#ifdef MPDATA_SINGLE
  call note(mpdata_plan_column_scan_f32_c(plan, sl0, n, int(tn, c_int), int(t1, c_int), c_loc(wgt_c), c_loc(total_c), &
                                          MPDATA_COLUMN_SCAN_DOWN), 'scan_host')
#else
  call note(mpdata_plan_column_scan_c(plan, sl0, n, int(tn, c_int), int(t1, c_int), c_loc(wgt_c), c_loc(total_c), &
                                      MPDATA_COLUMN_SCAN_DOWN), 'scan_host')
#endif
  call put_r('total_c', total_c, shape(total_c))

  ! ---- refused: an unknown mode bit
  call note(mpdata_plan_column_scan_device_c(plan, 0_c_int64_t, ncrms, int(t1, c_int), int(tn, c_int), c_null_ptr, c_null_ptr, &
                                             4_c_int), 'scan_badmode')

  call calls_close()
  call dfree(d_wgt); call dfree(d_total)
end program column_scan_calls
