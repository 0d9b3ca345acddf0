! vsolve_calls.F90 -- a TEST program: the implicit vertical solve of a resident plan's tracers (include/mpdata_hip.h
! section 3o) driven from Fortran through the interfaces of mpdata_hip_mod alone.  It has no oracle and no interface block
! of its own for a library name.
!
!   ./vsolve_calls <input file> <dump file>       (vsolve_calls_sp: the -DMPDATA_SINGLE build, rp = c_float)
!
! Both files are streams of records in the format of calls_common.F90, which holds the helpers and the frame around the
! calls below as well (calls_open, calls_import, calls_close).  The input file is written by tests/test_plan_vsolve.py,
! which replays the script on the numpy model and compares every record of the dump bit for bit, the return code of every
! call included: a code is recorded, never stopped on.
!
! The script: create, set_boundary(PERIODIC), import_device of all seven arrays - vsolve on the block (sl0, n), all
! tracers - read-back - vsolve on the whole plan, tracers [t1, t1+tn) - run - export_device - destroy.
program vsolve_calls
  use iso_c_binding
  use mpdata_grid
  use mpdata_hip_mod
  use calls_common
  implicit none
  real(rp), allocatable, target :: lo_a(:,:), di_a(:,:), up_a(:,:), lo_b(:,:), di_b(:,:), up_b(:,:)
  type(c_ptr) :: d_lo, d_di, d_up

  call calls_open('vsolve_calls')
  allocate(lo_a(n, nzm), di_a(n, nzm), up_a(n, nzm), lo_b(ncrms, nzm), di_b(ncrms, nzm), up_b(ncrms, nzm))
  call get_r('lo_a', lo_a, shape(lo_a)); call get_r('di_a', di_a, shape(di_a)); call get_r('up_a', up_a, shape(up_a))
  call get_r('lo_b', lo_b, shape(lo_b)); call get_r('di_b', di_b, shape(di_b)); call get_r('up_b', up_b, shape(up_b))
  call dalloc(d_lo, size(lo_b)); call dalloc(d_di, size(di_b)); call dalloc(d_up, size(up_b))
  call calls_import()

  ! ---- the block, all tracers; the read-back behind it
  call to_dev(d_lo, lo_a, size(lo_a)); call to_dev(d_di, di_a, size(di_a)); call to_dev(d_up, up_a, size(up_a))
  call note(mpdata_plan_vsolve_device_c(plan, sl0, n, d_lo, d_di, d_up, 0_c_int, int(T, c_int)), 'vs_block')
  call note(mpdata_plan_sync_c(plan), 'sync')
  fout = SENTINEL; fluxout = SENTINEL
  call to_dev(d_f, fout, size(fout)); call to_dev(d_flux, fluxout, size(fluxout))
  call note(mpdata_plan_export_device_c(plan, d_f, d_flux, 0_c_int, int(T, c_int)), 'export')
  call note(mpdata_plan_sync_c(plan), 'sync')
  call to_host(fout, d_f, size(fout)); call to_host(fluxout, d_flux, size(fluxout))
  call put_r('f_a', fout, shape(fout)); call put_r('flux_a', fluxout, shape(fluxout))

  ! ---- the whole plan, a tracer sub-range
  call to_dev(d_lo, lo_b, size(lo_b)); call to_dev(d_di, di_b, size(di_b)); call to_dev(d_up, up_b, size(up_b))
  call note(mpdata_plan_vsolve_device_c(plan, 0_c_int64_t, ncrms, d_lo, d_di, d_up, int(t1, c_int), int(tn, c_int)), 'vs_range')
  call note(mpdata_plan_sync_c(plan), 'sync')

  call calls_close()
  call dfree(d_lo); call dfree(d_di); call dfree(d_up)
end program vsolve_calls
