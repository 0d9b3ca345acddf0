! vdiffuse_calls.F90 -- a TEST program: the implicit vertical diffusion of a resident plan's tracers with a per-cell
! diffusivity (include/mpdata_hip.h section 3s) driven from Fortran through the interfaces of mpdata_hip_mod alone.  It has
! no oracle and no interface block of its own for a library name.
!
!   ./vdiffuse_calls <input file> <dump file>       (vdiffuse_calls_sp: the -DMPDATA_SINGLE build, rp = c_float)
!
! Both files are streams of records in the format of calls_common.F90, which holds the helpers and the frame around the
! calls below as well (calls_open, calls_import, calls_close).  The input file is written by tests/test_plan_vdiffuse.py,
! which replays the script on the numpy model and compares every record of the dump bit for bit, the return code of every
! call included: a code is recorded, never stopped on.
!
! The script: create, set_boundary(PERIODIC), import_device of all seven arrays - vdiffuse on the block (sl0, n), all
! tracers, with sb and st - read-back - vdiffuse on the whole plan, tracers [t1, t1+tn), without sb and st - run -
! export_device - destroy.
program vdiffuse_calls
  use iso_c_binding
  use mpdata_grid
  use mpdata_hip_mod
  use calls_common
  implicit none
  real(rp), allocatable, target :: tkh_a(:,:,:), cz_a(:,:), sb_a(:,:), st_a(:,:), tkh_b(:,:,:), cz_b(:,:)
  type(c_ptr) :: d_tkh, d_cz, d_sb, d_st

  call calls_open('vdiffuse_calls')
  allocate(tkh_a(n, 0:nx+1, nzm), cz_a(n, nzm), sb_a(n, nx), st_a(n, nx), tkh_b(ncrms, 0:nx+1, nzm), cz_b(ncrms, nzm))
  call get_r('tkh_a', tkh_a, shape(tkh_a)); call get_r('cz_a', cz_a, shape(cz_a))
  call get_r('sb_a', sb_a, shape(sb_a)); call get_r('st_a', st_a, shape(st_a))
  call get_r('tkh_b', tkh_b, shape(tkh_b)); call get_r('cz_b', cz_b, shape(cz_b))
  call dalloc(d_tkh, size(tkh_b)); call dalloc(d_cz, size(cz_b)); call dalloc(d_sb, size(sb_a)); call dalloc(d_st, size(st_a))
  call calls_import()

  ! ---- the block, all tracers, both boundary fluxes; the read-back behind it
  call to_dev(d_tkh, tkh_a, size(tkh_a)); call to_dev(d_cz, cz_a, size(cz_a))
  call to_dev(d_sb, sb_a, size(sb_a)); call to_dev(d_st, st_a, size(st_a))
  call note(mpdata_plan_vdiffuse_device_c(plan, sl0, n, d_tkh, d_cz, d_sb, d_st, 0_c_int, int(T, c_int)), 'vd_block')
  call note(mpdata_plan_sync_c(plan), 'sync')
  fout = SENTINEL; fluxout = SENTINEL
  call to_dev(d_f, fout, size(fout)); call to_dev(d_flux, fluxout, size(fluxout))
  call note(mpdata_plan_export_device_c(plan, d_f, d_flux, 0_c_int, int(T, c_int)), 'export')
  call note(mpdata_plan_sync_c(plan), 'sync')
  call to_host(fout, d_f, size(fout)); call to_host(fluxout, d_flux, size(fluxout))
  call put_r('f_a', fout, shape(fout)); call put_r('flux_a', fluxout, shape(fluxout))

  ! ---- the whole plan, a tracer sub-range, no boundary fluxes
  call to_dev(d_tkh, tkh_b, size(tkh_b)); call to_dev(d_cz, cz_b, size(cz_b))
  call note(mpdata_plan_vdiffuse_device_c(plan, 0_c_int64_t, ncrms, d_tkh, d_cz, c_null_ptr, c_null_ptr, int(t1, c_int), &
                                          int(tn, c_int)), 'vd_range')
  call note(mpdata_plan_sync_c(plan), 'sync')

  call calls_close()
  call dfree(d_tkh); call dfree(d_cz); call dfree(d_sb); call dfree(d_st)
end program vdiffuse_calls
