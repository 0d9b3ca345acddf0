! sediment_calls.F90 -- a TEST program: the sedimentation of a resident plan's tracers (include/mpdata_hip.h section 3n)
! driven from Fortran through the interfaces of mpdata_hip_mod alone.  It has no oracle and no interface block of its
! own for a library name.
!
!   ./sediment_calls <input file> <dump file>       (sediment_calls_sp: the -DMPDATA_SINGLE build, rp = c_float)
!
! Both files are streams of records in the format of calls_common.F90, which holds the helpers and the frame around the
! calls below as well (calls_open, calls_import, calls_close).  The input file is written by tests/test_plan_sediment.py,
! which replays the script on the numpy model and compares every record of the dump bit for bit, the return code of every
! call included: a code is recorded, never stopped on.
!
! The script: create, set_boundary(PERIODIC), import_device of all seven arrays - sediment on the block (sl0, n), all
! tracers, with psfc and pflux - sediment on the whole plan, tracers [t1, t1+tn), psfc and pflux null - run -
! export_device - destroy.
program sediment_calls
  use iso_c_binding
  use mpdata_grid
  use mpdata_hip_mod
  use calls_common
  implicit none
  real(rp), allocatable, target :: wp_a(:,:,:,:), wp_b(:,:,:,:), psfc(:,:,:), pflux(:,:,:)
  type(c_ptr) :: d_wp, d_psfc, d_pflux

  call calls_open('sediment_calls')
  allocate(wp_a(n, nx, nzm, T), wp_b(ncrms, nx, nzm, tn), psfc(n, nx, T), pflux(n, nzm, T))
  call get_r('wp_a', wp_a, shape(wp_a)); call get_r('wp_b', wp_b, shape(wp_b))
  call dalloc(d_wp, max(size(wp_a), size(wp_b))); call dalloc(d_psfc, size(psfc)); call dalloc(d_pflux, size(pflux))
  call calls_import()

  ! ---- the block, all tracers, with psfc and pflux
  psfc = SENTINEL; pflux = SENTINEL
  call to_dev(d_wp, wp_a, size(wp_a)); call to_dev(d_psfc, psfc, size(psfc)); call to_dev(d_pflux, pflux, size(pflux))
  call note(mpdata_plan_sediment_device_c(plan, sl0, n, d_wp, d_psfc, d_pflux, 0_c_int, int(T, c_int)), 'sed_block')
  call note(mpdata_plan_sync_c(plan), 'sync')
  call to_host(psfc, d_psfc, size(psfc)); call put_r('psfc', psfc, shape(psfc))
  call to_host(pflux, d_pflux, size(pflux)); call put_r('pflux', pflux, shape(pflux))

  ! ---- the whole plan, a tracer sub-range, psfc and pflux null
  call to_dev(d_wp, wp_b, size(wp_b))
  call note(mpdata_plan_sediment_device_c(plan, 0_c_int64_t, ncrms, d_wp, c_null_ptr, c_null_ptr, int(t1, c_int), &
            int(tn, c_int)), 'sed_range')
  call note(mpdata_plan_sync_c(plan), 'sync')

  call calls_close()
  call dfree(d_wp); call dfree(d_psfc); call dfree(d_pflux)
end program sediment_calls
