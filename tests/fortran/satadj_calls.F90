! satadj_calls.F90 -- a TEST program: the saturation adjustment of a resident plan's tracers (include/mpdata_hip.h section
! 3y) driven from Fortran through the interfaces and the derived type of mpdata_hip_mod alone.  It has no oracle and no
! interface block of its own for a library name.
!
!   ./satadj_calls <input file> <dump file>       (satadj_calls_sp: the -DMPDATA_SINGLE build, rp = c_float)
!
! Both files are streams of records in the format of calls_common.F90, which holds the helpers and the frame around the
! calls below as well (calls_open, calls_import, calls_close).  The input file is written by tests/test_plan_satadj.py,
! which replays the script on the numpy model and compares every record of the dump bit for bit, the return code of every
! call included: a code is recorded, never stopped on.  Of `params`, t1 is the tracer th and tn the tracer tn here; the
! record `tracers` holds tq, tt and maxit of the two calls.  The curve is the test's curve of tests/satadj_model.py (PAR),
! the same decimal numbers: the struct is of doubles in both builds, which the records of rp could not carry.
!
! The script: create, set_boundary(PERIODIC), import_device of all seven arrays - satadj on the block (sl0, n) with
! MPDATA_SATADJ_ICE, gz, tt, ncld and iters - satadj on the whole plan without ICE and tt, with gz, the second maxit, ncld
! and iters - a call with tn == tq, which is refused - run - export_device - destroy.
program satadj_calls
  use iso_c_binding
  use mpdata_grid
  use mpdata_hip_mod
  use calls_common
  implicit none
  real(rp), allocatable, target :: pres_a(:,:), gz_a(:,:), pres_b(:,:), gz_b(:,:), ncld_a(:,:), iters_a(:,:), ncld_b(:,:), iters_b(:,:)
  type(c_ptr) :: d_pres, d_gz, d_ncld, d_iters
  type(mpdata_satadj_params), target :: par
  integer(c_int64_t) :: tr(4)
  integer(c_int) :: th, tq, tc, tt

  call calls_open('satadj_calls')
  call get_i8('tracers', tr, [4])
  th = int(t1, c_int); tq = int(tr(1), c_int); tc = int(tn, c_int); tt = int(tr(2), c_int)
  allocate(pres_a(n, nzm), gz_a(n, nzm), pres_b(ncrms, nzm), gz_b(ncrms, nzm))
  allocate(ncld_a(n, nzm), iters_a(n, nzm), ncld_b(ncrms, nzm), iters_b(ncrms, nzm))
  call get_r('pres_a', pres_a, shape(pres_a)); call get_r('gz_a', gz_a, shape(gz_a))
  call get_r('pres_b', pres_b, shape(pres_b)); call get_r('gz_b', gz_b, shape(gz_b))
  call dalloc(d_pres, size(pres_b)); call dalloc(d_gz, size(gz_b)); call dalloc(d_ncld, size(ncld_b)); call dalloc(d_iters, size(iters_b))
  call calls_import()

  par%esw = [6.11239921d0, 0.443987641d0, 0.142986287d-1, 0.264847430d-3, 0.302950461d-5, 0.206739458d-7, 0.640689451d-10, &
             -0.952447341d-13, -0.976195544d-15]
  par%desw = [0.443956472d0, 0.285976452d-1, 0.794747212d-3, 0.121167162d-4, 0.103167413d-6, 0.385208005d-9, -0.604119582d-12, &
              -0.792933209d-14, -0.599634321d-17]
  par%esi = [6.11147274d0, 0.503160820d0, 0.188439774d-1, 0.420895665d-3, 0.615021634d-5, 0.602588177d-7, 0.385852041d-9, &
             0.146898966d-11, 0.252751365d-14]
  par%desi = [0.503223089d0, 0.377174432d-1, 0.126710138d-2, 0.249065913d-4, 0.312668753d-6, 0.255653718d-8, 0.132073448d-10, &
              0.390204672d-13, 0.497275778d-16]
  par%t0 = 273.16d0; par%xmin = -80.0d0; par%eps = 0.622d0
  par%lv = 2.5104d6 / 1004.0d0; par%ls = 2.8440d6 / 1004.0d0
  par%tmin = 253.16d0; par%tmax = 273.16d0; par%tol = 0.01d0

  ! ---- the block: ICE, gz, tt, both outputs
  par%maxit = int(tr(3), c_int)
  ncld_a = SENTINEL; iters_a = SENTINEL
  call to_dev(d_pres, pres_a, size(pres_a)); call to_dev(d_gz, gz_a, size(gz_a))
  call to_dev(d_ncld, ncld_a, size(ncld_a)); call to_dev(d_iters, iters_a, size(iters_a))
  call note(mpdata_plan_satadj_device_c(plan, sl0, n, th, tq, tc, tt, d_pres, d_gz, c_loc(par), MPDATA_SATADJ_ICE, d_ncld, d_iters), &
            'satadj_block')
  call note(mpdata_plan_sync_c(plan), 'sync')
  call to_host(ncld_a, d_ncld, size(ncld_a)); call put_r('ncld_a', ncld_a, shape(ncld_a))
  call to_host(iters_a, d_iters, size(iters_a)); call put_r('iters_a', iters_a, shape(iters_a))

  ! ---- the whole plan: liquid only, no tt, the second maxit
  par%maxit = int(tr(4), c_int)
  ncld_b = SENTINEL; iters_b = SENTINEL
  call to_dev(d_pres, pres_b, size(pres_b)); call to_dev(d_gz, gz_b, size(gz_b))
  call to_dev(d_ncld, ncld_b, size(ncld_b)); call to_dev(d_iters, iters_b, size(iters_b))
  call note(mpdata_plan_satadj_device_c(plan, 0_c_int64_t, ncrms, th, tq, tc, -1_c_int, d_pres, d_gz, c_loc(par), 0_c_int, &
                                        d_ncld, d_iters), 'satadj_whole')
  call note(mpdata_plan_sync_c(plan), 'sync')
  call to_host(ncld_b, d_ncld, size(ncld_b)); call put_r('ncld_b', ncld_b, shape(ncld_b))
  call to_host(iters_b, d_iters, size(iters_b)); call put_r('iters_b', iters_b, shape(iters_b))

  ! ---- refused: the same tracer twice
  call note(mpdata_plan_satadj_device_c(plan, 0_c_int64_t, ncrms, th, tq, tq, -1_c_int, d_pres, c_null_ptr, c_loc(par), 0_c_int, &
                                        c_null_ptr, c_null_ptr), 'satadj_same')

  call calls_close()
  call dfree(d_pres); call dfree(d_gz); call dfree(d_ncld); call dfree(d_iters)
end program satadj_calls
