! calls_common.F90 -- what the TEST programs tests/fortran/*_calls.F90 share, once: the record streams, the device copies and
! the frame of the six single-call programs.  Like the programs it reaches the library through mpdata_hip_mod alone; the two
! names of the HIP runtime below are the only bind(C) interfaces under tests/fortran/ beside advect_vs_cpu.F90.
!
! The record format of both files of a program: name (16 characters), element kind (int32: 1 int32, 2 int64, 3 real32,
! 4 real64), rank (int32), dims (int64 each), data.  A dump ends with the record `end` (kind 1, rank 0).
! tests/fortran_records.py writes and reads the same format.
!
! The frame, in three calls, so that a program's own reads, allocations and frees stand where they always stood:
!   calls_open(name)   the two files of the command line; `params` (8 x int64: ncrms, nx, nz, T, sl0, n, t1, tn), grid_set,
!                      the seven arrays of a plan and their device arrays.  The input file stays open for the program's own
!                      records, which it reads, and whose device arrays it allocates, next.
!   calls_import()     closes the input file and leaves a PERIODIC plan filled from the device arrays:
!                      rc:set_variant, rc:create, rc:set_boundary, rc:import
!   calls_close()      a step and the read-back: rc:run, rc:sync, rc:export, rc:sync, f_e, flux_e, rc:destroy; frees the seven
!                      device arrays, writes `end` and closes the dump.  The program frees its own device arrays behind it.
! plan_calls.F90 has a script of its own and takes the helpers only.
module calls_common
  use iso_c_binding
  use mpdata_grid
  use mpdata_hip_mod
  implicit none
  interface
    ! the programs' own copies to and from the device (codesign-kernels_amd/fortran/nested_hip.F90 is the precedent)
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
#ifdef MPDATA_SINGLE
  integer(c_int), parameter :: RKIND_CODE = 3
#else
  integer(c_int), parameter :: RKIND_CODE = 4
#endif
  real(rp), parameter :: SENTINEL = -777.0_rp
  integer, parameter :: UIN = 21, UOUT = 22
  integer(c_size_t), parameter :: EB = int(storage_size(1.0_rp) / 8, c_size_t)

  ! ---- the frame's state (adz is mpdata_grid's)
  integer(c_int64_t) :: ncrms, sl0, n
  integer :: T, t1, tn
  type(c_ptr) :: plan
  real(rp), allocatable, target :: f(:,:,:,:), u(:,:,:), w(:,:,:), rho(:,:), rhow(:,:), flux(:,:,:)
  real(rp), allocatable, target :: fout(:,:,:,:), fluxout(:,:,:)
  type(c_ptr) :: d_f, d_u, d_w, d_rho, d_rhow, d_adz, d_flux

contains

  !> the files of the command line, the plan's inputs and their device arrays
  subroutine calls_open(usage_name)
    character(*), intent(in) :: usage_name
    character(len=512) :: infile, outfile
    integer(c_int64_t) :: prm(8)
    if (command_argument_count() < 2) error stop 'usage: ' // usage_name // ' <input file> <dump file>'
    call get_command_argument(1, infile)
    call get_command_argument(2, outfile)
    open(unit=UIN, file=trim(infile), access='stream', form='unformatted', status='old')
    open(unit=UOUT, file=trim(outfile), access='stream', form='unformatted', status='replace')

    call get_i8('params', prm, [8])
    ncrms = prm(1); T = int(prm(4)); sl0 = prm(5); n = prm(6); t1 = int(prm(7)); tn = int(prm(8))
    call grid_set(ncrms, int(prm(2)), int(prm(3)), T)

    allocate(f(ncrms, -2:nx+3, nzm, T), u(ncrms, -1:nx+3, nzm), w(ncrms, -1:nx+2, nz), rho(ncrms, nzm), rhow(ncrms, nz), &
             flux(ncrms, nz, T))
    allocate(fout(ncrms, -2:nx+3, nzm, T), fluxout(ncrms, nz, T))
    call get_r('f', f, shape(f));       call get_r('u', u, shape(u));          call get_r('w', w, shape(w))
    call get_r('rho', rho, shape(rho)); call get_r('rhow', rhow, shape(rhow)); call get_r('adz', adz, shape(adz))
    call get_r('flux', flux, shape(flux))

    call dalloc(d_f, size(f)); call dalloc(d_u, size(u)); call dalloc(d_w, size(w)); call dalloc(d_rho, size(rho))
    call dalloc(d_rhow, size(rhow)); call dalloc(d_adz, size(adz)); call dalloc(d_flux, size(flux))
  end subroutine calls_open

  !> the plan, filled from device arrays
  subroutine calls_import()
    close(UIN)
    call note(mpdata_set_variant(0_c_int), 'set_variant')
    plan = c_null_ptr
    call note(mpdata_plan_create_c(nslices, nx, nz, ntracers, plan), 'create')
    if (.not. c_associated(plan)) error stop 'no plan'
    call note(mpdata_plan_set_boundary_c(plan, MPDATA_BOUNDARY_PERIODIC), 'set_boundary')
    call to_dev(d_f, f, size(f)); call to_dev(d_u, u, size(u)); call to_dev(d_w, w, size(w)); call to_dev(d_rho, rho, size(rho))
    call to_dev(d_rhow, rhow, size(rhow)); call to_dev(d_adz, adz, size(adz)); call to_dev(d_flux, flux, size(flux))
    call note(mpdata_plan_import_device_c(plan, d_f, d_u, d_w, d_rho, d_rhow, d_adz, d_flux, 0_c_int, int(T, c_int)), 'import')
  end subroutine calls_import

  !> a step on the new tracers, the read-back, and the end of the dump
  subroutine calls_close()
    character(len=16) :: tag
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
    tag = 'end'
    write(UOUT) tag, 1_c_int, 0_c_int
    close(UOUT)
  end subroutine calls_close

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

end module calls_common
