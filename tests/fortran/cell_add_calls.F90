! cell_add_calls.F90 -- a TEST program: the per-cell sources of a resident plan's tracers (include/mpdata_hip.h section 3p)
! driven from Fortran through the interfaces of mpdata_hip_mod alone.  It has no oracle and no interface block of its
! own for a library name.
!
!   ./cell_add_calls <input file> <dump file>       (cell_add_calls_sp: the -DMPDATA_SINGLE build, rp = c_float)
!
! Both files are streams of records in the format of calls_common.F90, which holds the helpers and the frame around the
! calls below as well (calls_open, calls_import, calls_close).  The input file is written by tests/test_plan_cell_add.py,
! which replays the script on the numpy model and compares every record of the dump bit for bit, the return code of every
! call included: a code is recorded, never stopped on.
!
! The script: create, set_boundary(PERIODIC), import_device of all seven arrays - cell_add on the block (sl0, n), all
! tracers, c = 0.75, clipped, with dsum - cell_add on the whole plan, tracers [t1, t1+tn), c = 0.1 (no fp32 number: the
! library rounds it once), not clipped, dsum null - run - export_device - destroy.
program cell_add_calls
  use iso_c_binding
  use mpdata_grid
  use mpdata_hip_mod
  use calls_common
  implicit none
  real(rp), allocatable, target :: s_a(:,:,:,:), s_b(:,:,:,:), dsum(:,:,:)
  type(c_ptr) :: d_s, d_dsum

  call calls_open('cell_add_calls')
  allocate(s_a(n, nx, nzm, T), s_b(ncrms, nx, nzm, tn), dsum(n, nzm, T))
  call get_r('s_a', s_a, shape(s_a)); call get_r('s_b', s_b, shape(s_b))
  call dalloc(d_s, max(size(s_a), size(s_b))); call dalloc(d_dsum, size(dsum))
  call calls_import()

  ! ---- the block, all tracers, clipped, with dsum
  dsum = SENTINEL
  call to_dev(d_s, s_a, size(s_a)); call to_dev(d_dsum, dsum, size(dsum))
  call note(mpdata_plan_cell_add_device_c(plan, sl0, n, d_s, 0.75_c_double, MPDATA_CELL_ADD_CLIP, d_dsum, 0_c_int, &
            int(T, c_int)), 'add_block')
  call note(mpdata_plan_sync_c(plan), 'sync')
  call to_host(dsum, d_dsum, size(dsum)); call put_r('dsum', dsum, shape(dsum))

  ! ---- the whole plan, a tracer sub-range, dsum null
  call to_dev(d_s, s_b, size(s_b))
  call note(mpdata_plan_cell_add_device_c(plan, 0_c_int64_t, ncrms, d_s, 0.1_c_double, MPDATA_CELL_ADD, c_null_ptr, &
            int(t1, c_int), int(tn, c_int)), 'add_range')
  call note(mpdata_plan_sync_c(plan), 'sync')

  call calls_close()
  call dfree(d_s); call dfree(d_dsum)
end program cell_add_calls
