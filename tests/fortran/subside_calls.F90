! subside_calls.F90 -- a TEST program: the large-scale vertical advection of a resident plan's tracers (include/mpdata_hip.h
! section 3m) driven from Fortran through the interfaces of mpdata_hip_mod alone.  It has no oracle and no interface block
! of its own for a library name.
!
!   ./subside_calls <input file> <dump file>       (subside_calls_sp: the -DMPDATA_SINGLE build, rp = c_float)
!
! Both files are streams of records in the format of calls_common.F90, which holds the helpers and the frame around the
! calls below as well (calls_open, calls_import, calls_close).  The input file is written by tests/test_plan_subside.py,
! which replays the script on the numpy model and compares every record of the dump bit for bit, the return code of every
! call included: a code is recorded, never stopped on.
!
! The script: create, set_boundary(PERIODIC), import_device of all seven arrays - subside on the block (sl0, n), all
! tracers, with dsum - subside on the whole plan, tracers [t1, t1+tn), dsum null - run - export_device - destroy.
program subside_calls
  use iso_c_binding
  use mpdata_grid
  use mpdata_hip_mod
  use calls_common
  implicit none
  real(rp), allocatable, target :: cb_a(:,:), cc_a(:,:), cb_b(:,:), cc_b(:,:), dsum(:,:,:)
  type(c_ptr) :: d_cb, d_cc, d_dsum

  call calls_open('subside_calls')
  allocate(cb_a(n, nzm), cc_a(n, nzm), cb_b(ncrms, nzm), cc_b(ncrms, nzm), dsum(n, nzm, T))
  call get_r('cb_a', cb_a, shape(cb_a)); call get_r('cc_a', cc_a, shape(cc_a))
  call get_r('cb_b', cb_b, shape(cb_b)); call get_r('cc_b', cc_b, shape(cc_b))
  call dalloc(d_cb, size(cb_b)); call dalloc(d_cc, size(cc_b)); call dalloc(d_dsum, size(dsum))
  call calls_import()

  ! ---- the block, all tracers, with dsum
  dsum = SENTINEL
  call to_dev(d_cb, cb_a, size(cb_a)); call to_dev(d_cc, cc_a, size(cc_a)); call to_dev(d_dsum, dsum, size(dsum))
  call note(mpdata_plan_subside_device_c(plan, sl0, n, d_cb, d_cc, d_dsum, 0_c_int, int(T, c_int)), 'subside_block')
  call note(mpdata_plan_sync_c(plan), 'sync')
  call to_host(dsum, d_dsum, size(dsum)); call put_r('dsum', dsum, shape(dsum))

  ! ---- the whole plan, a tracer sub-range, dsum null
  call to_dev(d_cb, cb_b, size(cb_b)); call to_dev(d_cc, cc_b, size(cc_b))
  call note(mpdata_plan_subside_device_c(plan, 0_c_int64_t, ncrms, d_cb, d_cc, c_null_ptr, int(t1, c_int), int(tn, c_int)), &
            'subside_range')
  call note(mpdata_plan_sync_c(plan), 'sync')

  call calls_close()
  call dfree(d_cb); call dfree(d_cc); call dfree(d_dsum)
end program subside_calls
