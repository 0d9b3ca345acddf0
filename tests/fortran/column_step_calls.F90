! column_step_calls.F90 -- a TEST program: the fused column step of a resident plan's tracers (include/mpdata_hip.h section
! 3q) driven from Fortran through the interfaces of mpdata_hip_mod alone.  It has no oracle and no interface block of its
! own for a library name.
!
!   ./column_step_calls <input file> <dump file>       (column_step_calls_sp: the -DMPDATA_SINGLE build, rp = c_float)
!
! Both files are streams of records in the format of plan_calls.F90: name (16 characters), element kind (int32: 1 int32,
! 2 int64, 3 real32, 4 real64), rank (int32), dims (int64 each), data.  The input file is written by
! tests/test_plan_column_step.py, which replays the script on the numpy model and compares every record of the dump bit
! for bit, the return code of every call included: a code is recorded, never stopped on.
!
! The script: create, set_boundary(PERIODIC), import_device of all seven arrays - all four stages on the block (sl0, n),
! all tracers, c = 0.75, clipped, with psfc - source and vsolve alone on the whole plan, tracers [t1, t1+tn), c = 0.1 (no
! fp32 number: the library rounds it once), not clipped - a call without a stage (refused) - run - export_device - destroy.
module column_step_calls_hip
  use iso_c_binding
  implicit none
  interface
    ! the program's own copies to and from the device (tests/fortran/plan_calls.F90 is the precedent)
    integer(c_int) function hipMemcpy(dst, src, bytes, kind) bind(C, name="hipMemcpy")
      import :: c_int, c_ptr, c_size_t
      type(c_ptr), value :: dst, src
      integer(c_size_t), value :: bytes
      integer(c_int), value :: kind      ! 1 host -> device, 2 device -> host
    end function
    integer(c_int) function hipDeviceSynchronize() bind(C, name="hipDeviceSynchronize")
      import :: c_int
    end function
  end interface
end module column_step_calls_hip

program column_step_calls
  use iso_c_binding
  use mpdata_grid
  use mpdata_hip_mod
  use column_step_calls_hip
  implicit none
#ifdef MPDATA_SINGLE
  integer(c_int), parameter :: RKIND_CODE = 3
#else
  integer(c_int), parameter :: RKIND_CODE = 4
#endif
  real(rp), parameter :: SENTINEL = -777.0_rp
  integer, parameter :: UIN = 21, UOUT = 22
  integer(c_size_t), parameter :: EB = int(storage_size(1.0_rp) / 8, c_size_t)

  character(len=512) :: infile, outfile
  character(len=16) :: tag
  integer(c_int64_t) :: prm(8), ncrms, sl0, n
  integer :: T, t1, tn
  type(c_ptr) :: plan
  real(rp), allocatable, target :: f(:,:,:,:), u(:,:,:), w(:,:,:), rho(:,:), rhow(:,:), flux(:,:,:)
  real(rp), allocatable, target :: s_a(:,:,:,:), s_b(:,:,:,:), wp(:,:,:,:), psfc(:,:,:)
  real(rp), allocatable, target :: cb(:,:), cc(:,:), lo_a(:,:), di_a(:,:), up_a(:,:), lo_b(:,:), di_b(:,:), up_b(:,:)
  real(rp), allocatable, target :: fout(:,:,:,:), fluxout(:,:,:)
  type(c_ptr) :: d_f, d_u, d_w, d_rho, d_rhow, d_adz, d_flux, d_s, d_wp, d_psfc, d_cb, d_cc, d_lo, d_di, d_up

  if (command_argument_count() < 2) error stop 'usage: column_step_calls <input file> <dump file>'
  call get_command_argument(1, infile)
  call get_command_argument(2, outfile)
  open(unit=UIN, file=trim(infile), access='stream', form='unformatted', status='old')
  open(unit=UOUT, file=trim(outfile), access='stream', form='unformatted', status='replace')

  call get_i8('params', prm, [8])
  ncrms = prm(1); T = int(prm(4)); sl0 = prm(5); n = prm(6); t1 = int(prm(7)); tn = int(prm(8))
  call grid_set(ncrms, int(prm(2)), int(prm(3)), T)

  allocate(f(ncrms, -2:nx+3, nzm, T), u(ncrms, -1:nx+3, nzm), w(ncrms, -1:nx+2, nz), rho(ncrms, nzm), rhow(ncrms, nz), &
           flux(ncrms, nz, T))
  allocate(s_a(n, nx, nzm, T), s_b(ncrms, nx, nzm, tn), wp(n, nx, nzm, T), psfc(n, nx, T))
  allocate(cb(n, nzm), cc(n, nzm), lo_a(n, nzm), di_a(n, nzm), up_a(n, nzm), lo_b(ncrms, nzm), di_b(ncrms, nzm), up_b(ncrms, nzm))
  allocate(fout(ncrms, -2:nx+3, nzm, T), fluxout(ncrms, nz, T))
  call get_r('f', f, shape(f));       call get_r('u', u, shape(u));          call get_r('w', w, shape(w))
  call get_r('rho', rho, shape(rho)); call get_r('rhow', rhow, shape(rhow)); call get_r('adz', adz, shape(adz))
  call get_r('flux', flux, shape(flux))
  call get_r('s_a', s_a, shape(s_a)); call get_r('s_b', s_b, shape(s_b)); call get_r('wp', wp, shape(wp))
  call get_r('cb', cb, shape(cb));       call get_r('cc', cc, shape(cc))
  call get_r('lo_a', lo_a, shape(lo_a)); call get_r('di_a', di_a, shape(di_a)); call get_r('up_a', up_a, shape(up_a))
  call get_r('lo_b', lo_b, shape(lo_b)); call get_r('di_b', di_b, shape(di_b)); call get_r('up_b', up_b, shape(up_b))
  close(UIN)

  call dalloc(d_f, size(f)); call dalloc(d_u, size(u)); call dalloc(d_w, size(w)); call dalloc(d_rho, size(rho))
  call dalloc(d_rhow, size(rhow)); call dalloc(d_adz, size(adz)); call dalloc(d_flux, size(flux))
  call dalloc(d_s, max(size(s_a), size(s_b))); call dalloc(d_wp, size(wp)); call dalloc(d_psfc, size(psfc))
  call dalloc(d_cb, size(cb)); call dalloc(d_cc, size(cc))
  call dalloc(d_lo, size(lo_b)); call dalloc(d_di, size(di_b)); call dalloc(d_up, size(up_b))

  ! ---- the plan, filled from device arrays
  call note(mpdata_set_variant(0_c_int), 'set_variant')
  plan = c_null_ptr
  call note(mpdata_plan_create_c(nslices, nx, nz, ntracers, plan), 'create')
  if (.not. c_associated(plan)) error stop 'no plan'
  call note(mpdata_plan_set_boundary_c(plan, MPDATA_BOUNDARY_PERIODIC), 'set_boundary')
  call to_dev(d_f, f, size(f)); call to_dev(d_u, u, size(u)); call to_dev(d_w, w, size(w)); call to_dev(d_rho, rho, size(rho))
  call to_dev(d_rhow, rhow, size(rhow)); call to_dev(d_adz, adz, size(adz)); call to_dev(d_flux, flux, size(flux))
  call note(mpdata_plan_import_device_c(plan, d_f, d_u, d_w, d_rho, d_rhow, d_adz, d_flux, 0_c_int, int(T, c_int)), 'import')

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

  ! ---- a step on the new tracers, and the read-back
  call note(mpdata_plan_run_c(plan), 'run')
  call note(mpdata_plan_sync_c(plan), 'sync')
  fout = SENTINEL; fluxout = SENTINEL
  call to_dev(d_f, fout, size(fout)); call to_dev(d_flux, fluxout, size(fluxout))
  call note(mpdata_plan_export_device_c(plan, d_f, d_flux, 0_c_int, int(T, c_int)), 'export')
  call note(mpdata_plan_sync_c(plan), 'sync')
  call to_host(fout, d_f, size(fout)); call to_host(fluxout, d_flux, size(fluxout))
  call put_r('f_e', fout, shape(fout)); call put_r('flux_e', fluxout, shape(fluxout))
  call note(mpdata_plan_destroy_c(plan), 'destroy')

  call dfree(d_f); call dfree(d_u); call dfree(d_w); call dfree(d_rho); call dfree(d_rhow); call dfree(d_adz); call dfree(d_flux)
  call dfree(d_s); call dfree(d_wp); call dfree(d_psfc); call dfree(d_cb); call dfree(d_cc); call dfree(d_lo); call dfree(d_di)
  call dfree(d_up)
  tag = 'end'
  write(UOUT) tag, 1_c_int, 0_c_int
  close(UOUT)

contains

  !> the return code of a call, as a record of its own
  subroutine note(code, what)
    integer(c_int), intent(in) :: code
    character(*), intent(in) :: what
    call put_i4('rc:' // what, [code], [1])
  end subroutine note

  subroutine header(name, kind, dims)
    character(*), intent(in) :: name
    integer(c_int), intent(in) :: kind
    integer, intent(in) :: dims(:)
    character(len=16) :: nm
    nm = name
    if (len_trim(name) > 16) error stop 'record name longer than 16 characters'
    write(UOUT) nm, kind, int(size(dims), c_int), int(dims, c_int64_t)
  end subroutine header

  subroutine put_r(name, a, dims)
    character(*), intent(in) :: name
    real(rp), intent(in) :: a(*)
    integer, intent(in) :: dims(:)
    call header(name, RKIND_CODE, dims)
    write(UOUT) a(1:product(dims))
  end subroutine put_r

  subroutine put_i4(name, a, dims)
    character(*), intent(in) :: name
    integer(c_int), intent(in) :: a(*)
    integer, intent(in) :: dims(:)
    call header(name, 1_c_int, dims)
    write(UOUT) a(1:product(dims))
  end subroutine put_i4

  !> the next record of the input file must be `name`, of kind `kind` and of exactly the shape `dims`
  subroutine expect(name, kind, dims)
    character(*), intent(in) :: name
    integer(c_int), intent(in) :: kind
    integer, intent(in) :: dims(:)
    character(len=16) :: nm
    integer(c_int) :: k, r
    integer(c_int64_t) :: d(7)
    read(UIN) nm, k, r
    if (trim(nm) /= name .or. k /= kind .or. r /= size(dims)) then
      write(*,*) 'input record ', trim(nm), k, r, ' where ', name, kind, size(dims), ' was expected'
      error stop 2
    end if
    read(UIN) d(1:r)
    if (any(d(1:r) /= dims)) then
      write(*,*) 'input record ', name, ' has the shape ', d(1:r), ', the program declares ', dims
      error stop 2
    end if
  end subroutine expect

  subroutine get_r(name, a, dims)
    character(*), intent(in) :: name
    real(rp), intent(out) :: a(*)
    integer, intent(in) :: dims(:)
    call expect(name, RKIND_CODE, dims)
    read(UIN) a(1:product(dims))
  end subroutine get_r

  subroutine get_i8(name, a, dims)
    character(*), intent(in) :: name
    integer(c_int64_t), intent(out) :: a(*)
    integer, intent(in) :: dims(:)
    call expect(name, 2_c_int, dims)
    read(UIN) a(1:product(dims))
  end subroutine get_i8

  subroutine dalloc(p, nelem)
    type(c_ptr), intent(out) :: p
    integer, intent(in) :: nelem
    p = c_null_ptr
    call mpdata_check(mpdata_device_alloc_c(p, int(max(nelem, 1), c_int64_t) * int(EB, c_int64_t)), 'mpdata_device_alloc')
  end subroutine dalloc

  subroutine dfree(p)
    type(c_ptr), intent(in) :: p
    call mpdata_check(mpdata_device_free_c(p), 'mpdata_device_free')
  end subroutine dfree

  !> nelem reals host -> device; the device is idle when this returns
  subroutine to_dev(p, a, nelem)
    type(c_ptr), intent(in) :: p
    real(rp), intent(in), target :: a(*)
    integer, intent(in) :: nelem
    if (nelem < 1) return
    if (hipMemcpy(p, c_loc(a), int(nelem, c_size_t) * EB, 1_c_int) /= 0) error stop 'hipMemcpy to the device failed'
    if (hipDeviceSynchronize() /= 0) error stop 'hipDeviceSynchronize failed'
  end subroutine to_dev

  subroutine to_host(a, p, nelem)
    real(rp), intent(inout), target :: a(*)
    type(c_ptr), intent(in) :: p
    integer, intent(in) :: nelem
    if (nelem < 1) return
    if (hipMemcpy(c_loc(a), p, int(nelem, c_size_t) * EB, 2_c_int) /= 0) error stop 'hipMemcpy to the host failed'
  end subroutine to_host

end program column_step_calls
