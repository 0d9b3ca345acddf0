! convert_calls.F90 -- a TEST program: the first-order conversion between two tracers of a resident plan (include/mpdata_hip.h
! section 3t) driven from Fortran through the interfaces of mpdata_hip_mod alone.  It has no oracle and no interface block
! of its own for a library name.
!
!   ./convert_calls <input file> <dump file>       (convert_calls_sp: the -DMPDATA_SINGLE build, rp = c_float)
!
! Both files are streams of records in the format of calls_common.F90, which holds the helpers and the frame around the
! calls below as well (calls_open, calls_import, calls_close).  The input file is written by tests/test_plan_convert.py,
! which replays the script on the numpy model and compares every record of the dump bit for bit, the return code of every
! call included: a code is recorded, never stopped on.  Of `params`, t1 is the tracer src and tn the tracer dst here.
!
! The script: create, set_boundary(PERIODIC), import_device of all seven arrays - convert src -> dst on the block (sl0, n)
! with q0, y and dsum - convert dst -> src on the whole plan with MPDATA_CONVERT_LIMIT, no q0, no y, with dsum - a call
! with src == dst, which is refused - run - export_device - destroy.
program convert_calls
  use iso_c_binding
  use mpdata_grid
  use mpdata_hip_mod
  use calls_common
  implicit none
  real(rp), allocatable, target :: r_a(:,:), q0_a(:,:), y_a(:,:), r_b(:,:), dsum_a(:,:), dsum_b(:,:)
  type(c_ptr) :: d_r, d_q0, d_y, d_dsum

  call calls_open('convert_calls')
  allocate(r_a(n, nzm), q0_a(n, nzm), y_a(n, nzm), r_b(ncrms, nzm), dsum_a(n, nzm), dsum_b(ncrms, nzm))
  call get_r('r_a', r_a, shape(r_a)); call get_r('q0_a', q0_a, shape(q0_a)); call get_r('y_a', y_a, shape(y_a))
  call get_r('r_b', r_b, shape(r_b))
  call dalloc(d_r, size(r_b)); call dalloc(d_q0, size(q0_a)); call dalloc(d_y, size(y_a)); call dalloc(d_dsum, size(dsum_b))
  call calls_import()

  ! ---- the block, src -> dst, threshold and yield, with dsum
  dsum_a = SENTINEL
  call to_dev(d_r, r_a, size(r_a)); call to_dev(d_q0, q0_a, size(q0_a)); call to_dev(d_y, y_a, size(y_a))
  call to_dev(d_dsum, dsum_a, size(dsum_a))
  call note(mpdata_plan_convert_device_c(plan, sl0, n, int(t1, c_int), int(tn, c_int), d_r, d_q0, d_y, 0_c_int, d_dsum), &
            'convert_block')
  call note(mpdata_plan_sync_c(plan), 'sync')
  call to_host(dsum_a, d_dsum, size(dsum_a)); call put_r('dsum_a', dsum_a, shape(dsum_a))

  ! ---- the whole plan, dst -> src, capped, no threshold, no yield
  dsum_b = SENTINEL
  call to_dev(d_r, r_b, size(r_b)); call to_dev(d_dsum, dsum_b, size(dsum_b))
  call note(mpdata_plan_convert_device_c(plan, 0_c_int64_t, ncrms, int(tn, c_int), int(t1, c_int), d_r, c_null_ptr, c_null_ptr, &
                                         MPDATA_CONVERT_LIMIT, d_dsum), 'convert_back')
  call note(mpdata_plan_sync_c(plan), 'sync')
  call to_host(dsum_b, d_dsum, size(dsum_b)); call put_r('dsum_b', dsum_b, shape(dsum_b))

  ! ---- refused: the same tracer twice
  call note(mpdata_plan_convert_device_c(plan, 0_c_int64_t, ncrms, int(t1, c_int), int(t1, c_int), d_r, c_null_ptr, c_null_ptr, &
                                         0_c_int, c_null_ptr), 'convert_same')

  call calls_close()
  call dfree(d_r); call dfree(d_q0); call dfree(d_y); call dfree(d_dsum)
end program convert_calls
