! plan_calls.F90 -- a TEST program: a resident plan driven from Fortran the way INTEGRATION.md section 2b tells a host model
! to, through the interfaces of mpdata_hip_mod alone (sections 3 - 3l and 4b of include/mpdata_hip.h).  It has no oracle and
! no interface block of its own for a library name: what it cannot reach through `use mpdata_hip_mod` it cannot call.  The
! arrays carry the Fortran shapes the module's comments promise, so the shapes are under test as well.
!
!   ./plan_calls <input file> <dump file>          (plan_calls_sp: the -DMPDATA_SINGLE build, rp = c_float)
!
! Both files are streams of records (the format, and the helpers that read and write it, are in calls_common.F90: name,
! element kind, rank, dims, data).  The input file is written by tests/test_fortran_plan_calls.py, which replays the same
! script on the numpy models and compares every record of the dump bit for bit, the return code of every call included: a
! code is recorded, never stopped on.  Outputs a call may leave alone are set to SENTINEL before the call.
!
! The script.  Every block call takes (sl0, n) from the input file; the instance calls take (bsl0, bn).
!   1. [switches] create, set_boundary(PERIODIC), upload; boundary, level_windows
!   2. S steps: import u, w (the other pointers null) - Courant number (host form on odd steps, device form on even ones) -
!      ncycle = max(1, ceiling(cinst / cmax)), su = sw = 1 / ncycle - scale_uw (step 1: host form; step 2: device form; step
!      3 and later: host form with sw null, the Courant number again (clev null), device form with su null) - maxval(ncycle)
!      runs - diffuse (device form: tracers [0, T-1) with sb, st, zflux, then the last tracer with sb null; step 2: the host
!      form, all tracers) - level_stats (device form with mx null, host form) - level_add (CLIP, device form, tracers
!      [t1, t1+tn); ADD, host form) - column_path (device form, mass null on step 1; host form) -
!      export_instances_device, download_instances, the exported f times 0.75, import_instances_device
!   3. export_device, download, last_kernel_ms, destroy
!   4. the array forms on reference-layout device arrays of the same problem: level_stats, level_add (CLIP), diffuse on
!      (sl0, n), column_path, courant, scale_uw, periodic_halo
program plan_calls
  use iso_c_binding
  use mpdata_grid
  use mpdata_hip_mod
  ! the shared helpers only: the frame of the single-call programs (their plan and arrays) stays out, this script has its own
  use calls_common, only: SENTINEL, UIN, UOUT, note, put_r, put_i4, get_r, get_i8, dalloc, dfree, to_dev, to_host, &
                          hipDeviceSynchronize
  implicit none
  real(rp), parameter :: FACTOR = 0.75_rp

  character(len=512) :: infile, outfile
  character(len=16) :: tag
  integer(c_int64_t) :: prm(13), ncrms, sl0, n, bsl0, bn
  integer :: T, S, t1, tn, odd, tall, step, ic, i, nrun, rcrun
  integer(c_int) :: rc
  real(rp) :: cmax(1)
  real(c_double) :: ms
  type(c_ptr) :: plan
  ! the plan's arrays (adz is mpdata_grid's), the velocities of every step, the block's inputs of every step
  real(rp), allocatable, target :: f(:,:,:,:), u(:,:,:), w(:,:,:), rho(:,:), rhow(:,:), flux(:,:,:)
  real(rp), allocatable, target :: us(:,:,:,:), ws(:,:,:,:)
  real(rp), allocatable, target :: tkh(:,:,:,:), cx(:,:,:), cz(:,:,:), sb(:,:,:), st(:,:,:)
  real(rp), allocatable, target :: dclip(:,:,:,:), dadd(:,:,:,:)
  real(rp), allocatable, target :: ad(:,:,:), asu(:), asw(:)
  ! outputs, in the shapes the module documents
  real(rp), allocatable, target :: clev(:,:), cinst(:), su(:), sw(:)
  real(rp), allocatable, target :: zflux_a(:,:,:), zflux_b(:,:,:), zflux(:,:,:)
  real(rp), allocatable, target :: fsum(:,:,:), fmin(:,:,:), fmax(:,:,:)
  real(rp), allocatable, target :: path(:,:,:), mass(:,:)
  real(rp), allocatable, target :: fb(:,:,:,:), fluxb(:,:,:), fout(:,:,:,:), fluxout(:,:,:)
  real(rp), allocatable, target :: asum(:,:,:), amin(:,:,:), amax(:,:,:), apath(:,:,:), amass(:,:), aclev(:,:), acinst(:)
  real(rp), allocatable, target :: azflux(:,:,:)
  integer(c_int), allocatable :: ncycle(:)
  ! device arrays (mpdata_device_alloc_c)
  type(c_ptr) :: d_f, d_u, d_w, d_rho, d_adz, d_flux, d_clev, d_cinst, d_su, d_sw, d_tkh, d_cx, d_cz, d_sb, d_st, d_zflux, &
                 d_sum, d_min, d_max, d_d, d_path, d_mass, d_fb, d_fluxb

  if (command_argument_count() < 2) error stop 'usage: plan_calls <input file> <dump file>'
  call get_command_argument(1, infile)
  call get_command_argument(2, outfile)
  open(unit=UIN, file=trim(infile), access='stream', form='unformatted', status='old')
  open(unit=UOUT, file=trim(outfile), access='stream', form='unformatted', status='replace')

  call get_i8('params', prm, [13])
  ncrms = prm(1); T = int(prm(4))
  sl0 = prm(5); n = prm(6); bsl0 = prm(7); bn = prm(8); S = int(prm(9)); t1 = int(prm(10)); tn = int(prm(11))
  odd = int(prm(12)); tall = int(prm(13))
  call grid_set(ncrms, int(prm(2)), int(prm(3)), T)
  call get_r('cmax', cmax, [1])

  allocate(f(ncrms, -2:nx+3, nzm, T), u(ncrms, -1:nx+3, nzm), w(ncrms, -1:nx+2, nz), rho(ncrms, nzm), rhow(ncrms, nz), &
           flux(ncrms, nz, T))
  allocate(us(ncrms, -1:nx+3, nzm, S), ws(ncrms, -1:nx+2, nz, S))
  allocate(tkh(n, 0:nx+1, nzm, S), cx(n, nzm, S), cz(n, nzm, S), sb(n, nx, S), st(n, nx, S))
  allocate(dclip(n, nzm, tn, S), dadd(n, nzm, T, S), ad(ncrms, nzm, T), asu(ncrms), asw(ncrms))
  allocate(clev(n, nzm), cinst(n), su(n), sw(n), ncycle(n))
  allocate(zflux_a(n, nz, max(T-1, 1)), zflux_b(n, nz, 1), zflux(n, nz, T))
  allocate(fsum(n, nzm, T), fmin(n, nzm, T), fmax(n, nzm, T), path(n, nx, T), mass(n, T))
  allocate(fb(bn, -2:nx+3, nzm, T), fluxb(bn, nz, T), fout(ncrms, -2:nx+3, nzm, T), fluxout(ncrms, nz, T))
  allocate(asum(ncrms, nzm, T), amin(ncrms, nzm, T), amax(ncrms, nzm, T), apath(ncrms, nx, T), amass(ncrms, T), &
           aclev(ncrms, nzm), acinst(ncrms), azflux(n, nz, T))
  call get_r('f', f, shape(f));       call get_r('u', u, shape(u));          call get_r('w', w, shape(w))
  call get_r('rho', rho, shape(rho)); call get_r('rhow', rhow, shape(rhow)); call get_r('adz', adz, shape(adz))
  call get_r('flux', flux, shape(flux))
  call get_r('us', us, shape(us));    call get_r('ws', ws, shape(ws))
  call get_r('tkh', tkh, shape(tkh)); call get_r('cx', cx, shape(cx));       call get_r('cz', cz, shape(cz))
  call get_r('sb', sb, shape(sb));    call get_r('st', st, shape(st))
  call get_r('dclip', dclip, shape(dclip)); call get_r('dadd', dadd, shape(dadd))
  call get_r('ad', ad, shape(ad));    call get_r('asu', asu, shape(asu));    call get_r('asw', asw, shape(asw))
  close(UIN)

  call dalloc(d_f, size(f)); call dalloc(d_u, size(u)); call dalloc(d_w, size(w)); call dalloc(d_rho, size(rho))
  call dalloc(d_adz, size(adz)); call dalloc(d_flux, size(flux))
  call dalloc(d_clev, size(aclev)); call dalloc(d_cinst, size(acinst)); call dalloc(d_su, size(asu)); call dalloc(d_sw, size(asw))
  call dalloc(d_tkh, size(tkh(:,:,:,1))); call dalloc(d_cx, size(cx(:,:,1))); call dalloc(d_cz, size(cz(:,:,1)))
  call dalloc(d_sb, size(sb(:,:,1))); call dalloc(d_st, size(st(:,:,1))); call dalloc(d_zflux, size(zflux))
  call dalloc(d_sum, size(asum)); call dalloc(d_min, size(amin)); call dalloc(d_max, size(amax)); call dalloc(d_d, size(ad))
  call dalloc(d_path, size(apath)); call dalloc(d_mass, size(amass)); call dalloc(d_fb, size(fb)); call dalloc(d_fluxb, size(fluxb))

  ! ---- 1. the plan
  call note(mpdata_set_variant(0_c_int), 'set_variant')
  if (odd /= 0) call note(mpdata_set_f32_odd_ncrms_c(1_c_int), 'set_f32_odd')
  if (tall /= 0) call note(mpdata_set_tall_columns_c(1_c_int), 'set_tall')
  plan = c_null_ptr
  call note(mpdata_plan_create_c(nslices, nx, nz, ntracers, plan), 'create')
  if (.not. c_associated(plan)) error stop 'no plan'
  call note(mpdata_plan_set_boundary_c(plan, MPDATA_BOUNDARY_PERIODIC), 'set_boundary')
  call note(mpdata_plan_upload_c(plan, f, u, w, rho, rhow, adz, flux), 'upload')
  call note(mpdata_plan_boundary_c(plan), 'boundary')
  call note(mpdata_plan_level_windows_c(plan), 'level_windows')

  ! ---- 2. the steps
  do step = 1, S
    call to_dev(d_u, us(:,:,:,step), size(u)); call to_dev(d_w, ws(:,:,:,step), size(w))
    call note(mpdata_plan_import_device_c(plan, c_null_ptr, d_u, d_w, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, 0_c_int, &
                                          int(T, c_int)), 'import_uw')
    ! the Courant number of the block
    clev = SENTINEL; cinst = SENTINEL
    if (mod(step, 2) == 1) then
      call note(mpdata_plan_courant_c(plan, sl0, n, c_loc(clev), c_loc(cinst)), 'courant_host')
    else
      call to_dev(d_clev, clev, size(clev)); call to_dev(d_cinst, cinst, size(cinst))
      call note(mpdata_plan_courant_device_c(plan, sl0, n, d_clev, d_cinst), 'courant_dev')
      call note(mpdata_plan_sync_c(plan), 'sync')
      call to_host(clev, d_clev, size(clev)); call to_host(cinst, d_cinst, size(cinst))
    end if
    call put_r('clev', clev, shape(clev)); call put_r('cinst', cinst, shape(cinst))
    do i = 1, int(n)
      ncycle(i) = max(1, ceiling(cinst(i) / cmax(1)))
      su(i) = 1.0_rp / real(ncycle(i), rp)
      sw(i) = su(i)
    end do
    call put_i4('ncycle', ncycle, shape(ncycle)); call put_r('su', su, shape(su))
    ! the velocities of the block divided by ncycle
    select case (step)
    case (1)
      call note(mpdata_plan_scale_uw_c(plan, sl0, n, c_loc(su), c_loc(sw)), 'scale_host')
    case (2)
      call to_dev(d_su, su, size(su)); call to_dev(d_sw, sw, size(sw))
      call note(mpdata_plan_scale_uw_device_c(plan, sl0, n, d_su, d_sw), 'scale_dev')
    case default
      call note(mpdata_plan_scale_uw_c(plan, sl0, n, c_loc(su), c_null_ptr), 'scale_host_u')
      ! (between the two: the Courant number of the scaled u and the unscaled w, clev null)
      cinst = SENTINEL
      call note(mpdata_plan_courant_c(plan, sl0, n, c_null_ptr, c_loc(cinst)), 'courant_mid')
      call put_r('cinst_mid', cinst, shape(cinst))
      call to_dev(d_sw, sw, size(sw))
      call note(mpdata_plan_scale_uw_device_c(plan, sl0, n, c_null_ptr, d_sw), 'scale_dev_w')
    end select
    nrun = maxval(ncycle); rcrun = 0
    do ic = 1, nrun
      rc = mpdata_plan_run_c(plan)
      if (rc /= 0) rcrun = rc
    end do
    call note(int(nrun, c_int), 'runs'); call note(int(rcrun, c_int), 'run')
    call note(mpdata_plan_sync_c(plan), 'sync')
    ! the eddy diffusion
    if (step == 2) then
      zflux = SENTINEL
      call note(mpdata_plan_diffuse_c(plan, sl0, n, c_loc(tkh(1,0,1,step)), c_loc(cx(1,1,step)), c_loc(cz(1,1,step)), &
                                      c_loc(sb(1,1,step)), c_loc(st(1,1,step)), c_loc(zflux)), 'diffuse_host')
      call put_r('zflux_h', zflux, shape(zflux))
    else
      call to_dev(d_tkh, tkh(:,:,:,step), size(tkh(:,:,:,step))); call to_dev(d_cx, cx(:,:,step), size(cx(:,:,step)))
      call to_dev(d_cz, cz(:,:,step), size(cz(:,:,step))); call to_dev(d_sb, sb(:,:,step), size(sb(:,:,step)))
      call to_dev(d_st, st(:,:,step), size(st(:,:,step)))
      if (T > 1) then
        zflux_a = SENTINEL; call to_dev(d_zflux, zflux_a, size(zflux_a))
        call note(mpdata_plan_diffuse_device_c(plan, sl0, n, d_tkh, d_cx, d_cz, d_sb, d_st, d_zflux, 0_c_int, int(T-1, c_int)), &
                  'diffuse_dev_a')
        call note(mpdata_plan_sync_c(plan), 'sync')
        call to_host(zflux_a, d_zflux, size(zflux_a)); call put_r('zflux_a', zflux_a, shape(zflux_a))
      end if
      zflux_b = SENTINEL; call to_dev(d_zflux, zflux_b, size(zflux_b))
      call note(mpdata_plan_diffuse_device_c(plan, sl0, n, d_tkh, d_cx, d_cz, c_null_ptr, d_st, d_zflux, int(T-1, c_int), &
                                             1_c_int), 'diffuse_dev_b')
      call note(mpdata_plan_sync_c(plan), 'sync')
      call to_host(zflux_b, d_zflux, size(zflux_b)); call put_r('zflux_b', zflux_b, shape(zflux_b))
    end if
    ! the horizontal statistics
    fsum = SENTINEL; fmin = SENTINEL
    call to_dev(d_sum, fsum, size(fsum)); call to_dev(d_min, fmin, size(fmin))
    call note(mpdata_plan_level_stats_device_c(plan, sl0, n, d_sum, d_min, c_null_ptr, 0_c_int, int(T, c_int)), 'stats_dev')
    call note(mpdata_plan_sync_c(plan), 'sync')
    call to_host(fsum, d_sum, size(fsum)); call to_host(fmin, d_min, size(fmin))
    call put_r('sum_d', fsum, shape(fsum)); call put_r('min_d', fmin, shape(fmin))
    fsum = SENTINEL; fmin = SENTINEL; fmax = SENTINEL
    call note(mpdata_plan_level_stats_c(plan, sl0, n, fsum, fmin, fmax), 'stats_host')
    call put_r('sum_h', fsum, shape(fsum)); call put_r('min_h', fmin, shape(fmin)); call put_r('max_h', fmax, shape(fmax))
    ! the increments
    call to_dev(d_d, dclip(:,:,:,step), size(dclip(:,:,:,step)))
    call note(mpdata_plan_level_add_device_c(plan, sl0, n, d_d, MPDATA_LEVEL_ADD_CLIP, int(t1, c_int), int(tn, c_int)), &
              'add_clip_dev')
    call note(mpdata_plan_sync_c(plan), 'sync')
    call note(mpdata_plan_level_add_c(plan, sl0, n, dadd(:,:,:,step), MPDATA_LEVEL_ADD), 'add_host')
    ! the column integrals
    path = SENTINEL; mass = SENTINEL
    call to_dev(d_path, path, size(path)); call to_dev(d_mass, mass, size(mass))
    if (step == 1) then
      call note(mpdata_plan_column_path_device_c(plan, sl0, n, d_path, c_null_ptr, 0_c_int, int(T, c_int)), 'path_dev')
    else
      call note(mpdata_plan_column_path_device_c(plan, sl0, n, d_path, d_mass, 0_c_int, int(T, c_int)), 'path_dev')
    end if
    call note(mpdata_plan_sync_c(plan), 'sync')
    call to_host(path, d_path, size(path)); call to_host(mass, d_mass, size(mass))
    call put_r('path_d', path, shape(path)); call put_r('mass_d', mass, shape(mass))
    path = SENTINEL; mass = SENTINEL
    call note(mpdata_plan_column_path_c(plan, sl0, n, c_loc(path), c_loc(mass)), 'path_host')
    call put_r('path_h', path, shape(path)); call put_r('mass_h', mass, shape(mass))
    ! a block of instances out, changed, and in again
    fb = SENTINEL; fluxb = SENTINEL
    call to_dev(d_fb, fb, size(fb)); call to_dev(d_fluxb, fluxb, size(fluxb))
    call note(mpdata_plan_export_instances_device_c(plan, bsl0, bn, d_fb, d_fluxb, 0_c_int, int(T, c_int)), 'export_block')
    call note(mpdata_plan_sync_c(plan), 'sync')
    call to_host(fb, d_fb, size(fb)); call to_host(fluxb, d_fluxb, size(fluxb))
    call put_r('f_eb', fb, shape(fb)); call put_r('flux_eb', fluxb, shape(fluxb))
    fb = SENTINEL; fluxb = SENTINEL
    call note(mpdata_plan_download_instances_c(plan, bsl0, bn, fb, fluxb), 'download_blk')
    call put_r('f_db', fb, shape(fb)); call put_r('flux_db', fluxb, shape(fluxb))
    fb = fb * FACTOR
    call to_dev(d_fb, fb, size(fb))
    call note(mpdata_plan_import_instances_device_c(plan, bsl0, bn, d_fb, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, &
                                                    c_null_ptr, c_null_ptr, 0_c_int, int(T, c_int)), 'import_block')
    call note(mpdata_plan_sync_c(plan), 'sync')
  end do

  ! ---- 3. the read-backs
  fout = SENTINEL; fluxout = SENTINEL
  call to_dev(d_f, fout, size(fout)); call to_dev(d_flux, fluxout, size(fluxout))
  call note(mpdata_plan_export_device_c(plan, d_f, d_flux, 0_c_int, int(T, c_int)), 'export')
  call note(mpdata_plan_sync_c(plan), 'sync')
  call to_host(fout, d_f, size(fout)); call to_host(fluxout, d_flux, size(fluxout))
  call put_r('f_e', fout, shape(fout)); call put_r('flux_e', fluxout, shape(fluxout))
  fout = SENTINEL; fluxout = SENTINEL
  call note(mpdata_plan_download_c(plan, fout, fluxout), 'download')
  call put_r('f_d', fout, shape(fout)); call put_r('flux_d', fluxout, shape(fluxout))
  ms = -1.0_c_double
  call note(mpdata_plan_last_kernel_ms_c(plan, ms), 'last_ms')
  call note(merge(1_c_int, 0_c_int, ms > 0.0_c_double), 'ms_positive')
  call note(mpdata_plan_destroy_c(plan), 'destroy')

  ! ---- 4. the array forms, on the arrays the plan was filled with
  call to_dev(d_f, f, size(f)); call to_dev(d_u, u, size(u)); call to_dev(d_w, w, size(w))
  call to_dev(d_rho, rho, size(rho)); call to_dev(d_adz, adz, size(adz))
  asum = SENTINEL; amin = SENTINEL; amax = SENTINEL
  call to_dev(d_sum, asum, size(asum)); call to_dev(d_min, amin, size(amin)); call to_dev(d_max, amax, size(amax))
  call note(mpdata_level_stats_device_c(nslices, nx, nz, ntracers, d_f, d_sum, d_min, d_max, c_null_ptr), 'a_stats')
  call to_dev(d_d, ad, size(ad))
  call note(mpdata_level_add_device_c(nslices, nx, nz, ntracers, d_f, d_d, MPDATA_LEVEL_ADD_CLIP, c_null_ptr), 'a_add')
  call to_dev(d_tkh, tkh(:,:,:,1), size(tkh(:,:,:,1))); call to_dev(d_cx, cx(:,:,1), size(cx(:,:,1)))
  call to_dev(d_cz, cz(:,:,1), size(cz(:,:,1))); call to_dev(d_sb, sb(:,:,1), size(sb(:,:,1)))
  call to_dev(d_st, st(:,:,1), size(st(:,:,1)))
  azflux = SENTINEL; call to_dev(d_zflux, azflux, size(azflux))
  call note(mpdata_diffuse_device_c(nslices, nx, nz, ntracers, sl0, n, d_f, d_rho, d_adz, d_tkh, d_cx, d_cz, d_sb, d_st, d_zflux, &
                                    c_null_ptr), 'a_diffuse')
  apath = SENTINEL; amass = SENTINEL
  call to_dev(d_path, apath, size(apath)); call to_dev(d_mass, amass, size(amass))
  call note(mpdata_column_path_device_c(nslices, nx, nz, ntracers, d_f, d_rho, d_adz, d_path, d_mass, c_null_ptr), 'a_path')
  aclev = SENTINEL; acinst = SENTINEL
  call to_dev(d_clev, aclev, size(aclev)); call to_dev(d_cinst, acinst, size(acinst))
  call note(mpdata_courant_device_c(nslices, nx, nz, d_u, d_w, d_rho, d_adz, d_clev, d_cinst, c_null_ptr), 'a_courant')
  call to_dev(d_su, asu, size(asu)); call to_dev(d_sw, asw, size(asw))
  call note(mpdata_scale_uw_device_c(nslices, nx, nz, d_u, d_w, d_su, d_sw, c_null_ptr), 'a_scale')
  call note(mpdata_periodic_halo_device_c(nslices, nx, nz, ntracers, d_f, d_u, d_w, c_null_ptr), 'a_halo')
  call note(hipDeviceSynchronize(), 'device_sync')
  call to_host(asum, d_sum, size(asum)); call to_host(amin, d_min, size(amin)); call to_host(amax, d_max, size(amax))
  call to_host(azflux, d_zflux, size(azflux)); call to_host(apath, d_path, size(apath)); call to_host(amass, d_mass, size(amass))
  call to_host(aclev, d_clev, size(aclev)); call to_host(acinst, d_cinst, size(acinst))
  call to_host(fout, d_f, size(fout)); call to_host(u, d_u, size(u)); call to_host(w, d_w, size(w))
  call put_r('a_sum', asum, shape(asum)); call put_r('a_min', amin, shape(amin)); call put_r('a_max', amax, shape(amax))
  call put_r('a_zflux', azflux, shape(azflux)); call put_r('a_path', apath, shape(apath)); call put_r('a_mass', amass, shape(amass))
  call put_r('a_clev', aclev, shape(aclev)); call put_r('a_cinst', acinst, shape(acinst))
  call put_r('a_f', fout, shape(fout)); call put_r('a_u', u, shape(u)); call put_r('a_w', w, shape(w))

  call dfree(d_f); call dfree(d_u); call dfree(d_w); call dfree(d_rho); call dfree(d_adz); call dfree(d_flux); call dfree(d_clev)
  call dfree(d_cinst); call dfree(d_su); call dfree(d_sw); call dfree(d_tkh); call dfree(d_cx); call dfree(d_cz); call dfree(d_sb)
  call dfree(d_st); call dfree(d_zflux); call dfree(d_sum); call dfree(d_min); call dfree(d_max); call dfree(d_d)
  call dfree(d_path); call dfree(d_mass); call dfree(d_fb); call dfree(d_fluxb)
  tag = 'end'
  write(UOUT) tag, 1_c_int, 0_c_int
  close(UOUT)

end program plan_calls
