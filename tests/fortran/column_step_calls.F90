! column_step_calls.F90 -- a TEST program: the fused column step of a resident plan's tracers (include/mpdata_hip.h section
! 3q) driven from Fortran through the interfaces of mpdata_hip_mod alone.  It has no oracle and no interface block of its
! own for a library name.
!
!   ./column_step_calls <input file> <dump file>       (column_step_calls_sp: the -DMPDATA_SINGLE build, rp = c_float)
!
! Both files are streams of records in the format of calls_common.F90, which holds the helpers and the frame around the
! calls below as well (calls_open, calls_import, calls_close).  The input file is written by
! tests/test_plan_column_step.py, which replays the script on the numpy model and compares every record of the dump bit
! for bit, the return code of every call included: a code is recorded, never stopped on.
!
! The script: create, set_boundary(PERIODIC), import_device of all seven arrays - all four stages on the block (sl0, n),
! all tracers, c = 0.75, clipped, with psfc - source and vsolve alone on the whole plan, tracers [t1, t1+tn), c = 0.1 (no
! fp32 number: the library rounds it once), not clipped - a call without a stage (refused) - run - export_device - destroy.
program column_step_calls
  use iso_c_binding
  use mpdata_grid
  use mpdata_hip_mod
  use calls_common
  implicit none
  real(rp), allocatable, target :: s_a(:,:,:,:), s_b(:,:,:,:), wp(:,:,:,:), psfc(:,:,:)
  real(rp), allocatable, target :: cb(:,:), cc(:,:), lo_a(:,:), di_a(:,:), up_a(:,:), lo_b(:,:), di_b(:,:), up_b(:,:)
  type(c_ptr) :: d_s, d_wp, d_psfc, d_cb, d_cc, d_lo, d_di, d_up

  call calls_open('column_step_calls')
  allocate(s_a(n, nx, nzm, T), s_b(ncrms, nx, nzm, tn), wp(n, nx, nzm, T), psfc(n, nx, T))
  allocate(cb(n, nzm), cc(n, nzm), lo_a(n, nzm), di_a(n, nzm), up_a(n, nzm), lo_b(ncrms, nzm), di_b(ncrms, nzm), up_b(ncrms, nzm))
  call get_r('s_a', s_a, shape(s_a)); call get_r('s_b', s_b, shape(s_b)); call get_r('wp', wp, shape(wp))
  call get_r('cb', cb, shape(cb));       call get_r('cc', cc, shape(cc))
  call get_r('lo_a', lo_a, shape(lo_a)); call get_r('di_a', di_a, shape(di_a)); call get_r('up_a', up_a, shape(up_a))
  call get_r('lo_b', lo_b, shape(lo_b)); call get_r('di_b', di_b, shape(di_b)); call get_r('up_b', up_b, shape(up_b))
  call dalloc(d_s, max(size(s_a), size(s_b))); call dalloc(d_wp, size(wp)); call dalloc(d_psfc, size(psfc))
  call dalloc(d_cb, size(cb)); call dalloc(d_cc, size(cc))
  call dalloc(d_lo, size(lo_b)); call dalloc(d_di, size(di_b)); call dalloc(d_up, size(up_b))
  call calls_import()

  ! ---- the block, all tracers, all four stages, clipped, with psfc
  psfc = SENTINEL
  call to_dev(d_s, s_a, size(s_a)); call to_dev(d_wp, wp, size(wp)); call to_dev(d_psfc, psfc, size(psfc))
  call to_dev(d_cb, cb, size(cb)); call to_dev(d_cc, cc, size(cc))
  call to_dev(d_lo, lo_a, size(lo_a)); call to_dev(d_di, di_a, size(di_a)); call to_dev(d_up, up_a, size(up_a))
  call note(mpdata_plan_column_step_device_c(plan, sl0, n, d_s, 0.75_c_double, MPDATA_CELL_ADD_CLIP, d_cb, d_cc, d_wp, d_psfc, &
            d_lo, d_di, d_up, 0_c_int, int(T, c_int)), 'step_block')
  call note(mpdata_plan_sync_c(plan), 'sync')
  call to_host(psfc, d_psfc, size(psfc)); call put_r('psfc', psfc, shape(psfc))

  ! ---- the whole plan, a tracer sub-range, the source and the solve alone
  call to_dev(d_s, s_b, size(s_b))
  call to_dev(d_lo, lo_b, size(lo_b)); call to_dev(d_di, di_b, size(di_b)); call to_dev(d_up, up_b, size(up_b))
  call note(mpdata_plan_column_step_device_c(plan, 0_c_int64_t, ncrms, d_s, 0.1_c_double, MPDATA_CELL_ADD, c_null_ptr, c_null_ptr, &
            c_null_ptr, c_null_ptr, d_lo, d_di, d_up, int(t1, c_int), int(tn, c_int)), 'step_range')
  call note(mpdata_plan_sync_c(plan), 'sync')

  ! ---- no stage: refused, nothing changes
  call note(mpdata_plan_column_step_device_c(plan, 0_c_int64_t, ncrms, c_null_ptr, 0.1_c_double, MPDATA_CELL_ADD, c_null_ptr, &
            c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, 0_c_int, int(T, c_int)), 'step_none')

  call calls_close()
  call dfree(d_s); call dfree(d_wp); call dfree(d_psfc); call dfree(d_cb); call dfree(d_cc); call dfree(d_lo); call dfree(d_di)
  call dfree(d_up)
end program column_step_calls
