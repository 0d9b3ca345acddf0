! relax_calls.F90 -- a TEST program: the relaxation of a resident plan's tracers to a level profile (include/mpdata_hip.h
! section 3r) driven from Fortran through the interfaces of mpdata_hip_mod alone.  It has no oracle and no interface block
! of its own for a library name.
!
!   ./relax_calls <input file> <dump file>       (relax_calls_sp: the -DMPDATA_SINGLE build, rp = c_float)
!
! Both files are streams of records in the format of calls_common.F90, which holds the helpers and the frame around the
! calls below as well (calls_open, calls_import, calls_close).  The input file is written by tests/test_plan_relax.py,
! which replays the script on the numpy model and compares every record of the dump bit for bit, the return code of every
! call included: a code is recorded, never stopped on.
!
! The script: create, set_boundary(PERIODIC), import_device of all seven arrays - relax on the block (sl0, n), all
! tracers, to the horizontal mean (target null), with mean - relax on the whole plan, tracers [t1, t1+tn), to a given
! target, with mean (which must come back as the target) - run - export_device - destroy.
program relax_calls
  use iso_c_binding
  use mpdata_grid
  use mpdata_hip_mod
  use calls_common
  implicit none
  real(rp), allocatable, target :: c_a(:,:), c_b(:,:), tgt_b(:,:,:), mean_a(:,:,:), mean_b(:,:,:)
  type(c_ptr) :: d_c, d_tgt, d_mean

  call calls_open('relax_calls')
  allocate(c_a(n, nzm), c_b(ncrms, nzm), tgt_b(ncrms, nzm, tn), mean_a(n, nzm, T), mean_b(ncrms, nzm, tn))
  call get_r('c_a', c_a, shape(c_a)); call get_r('c_b', c_b, shape(c_b)); call get_r('tgt_b', tgt_b, shape(tgt_b))
  call dalloc(d_c, max(size(c_a), size(c_b))); call dalloc(d_tgt, size(tgt_b))
  call dalloc(d_mean, max(size(mean_a), size(mean_b)))
  call calls_import()

  ! ---- the block, all tracers, to the horizontal mean, with mean
  mean_a = SENTINEL
  call to_dev(d_c, c_a, size(c_a)); call to_dev(d_mean, mean_a, size(mean_a))
  call note(mpdata_plan_relax_device_c(plan, sl0, n, d_c, c_null_ptr, d_mean, 0_c_int, int(T, c_int)), 'relax_block')
  call note(mpdata_plan_sync_c(plan), 'sync')
  call to_host(mean_a, d_mean, size(mean_a)); call put_r('mean_a', mean_a, shape(mean_a))

  ! ---- the whole plan, a tracer sub-range, to a target; mean comes back as the target
  mean_b = SENTINEL
  call to_dev(d_c, c_b, size(c_b)); call to_dev(d_tgt, tgt_b, size(tgt_b)); call to_dev(d_mean, mean_b, size(mean_b))
  call note(mpdata_plan_relax_device_c(plan, 0_c_int64_t, ncrms, d_c, d_tgt, d_mean, int(t1, c_int), int(tn, c_int)), &
            'relax_range')
  call note(mpdata_plan_sync_c(plan), 'sync')
  call to_host(mean_b, d_mean, size(mean_b)); call put_r('mean_b', mean_b, shape(mean_b))

  call calls_close()
  call dfree(d_c); call dfree(d_tgt); call dfree(d_mean)
end program relax_calls
