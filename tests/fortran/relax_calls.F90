! relax_calls.F90 -- a TEST program: the relaxation of a resident plan's tracers to a level profile (include/mpdata_hip.h
! section 3r) driven from Fortran through the interfaces of mpdata_hip_mod alone.  It has no oracle and no interface block
! of its own for a library name.
!
!   ./relax_calls <input file> <dump file>       (relax_calls_sp: the -DMPDATA_SINGLE build, rp = c_float)
!
! Both files are streams of records in the format of plan_calls.F90: name (16 characters), element kind (int32: 1 int32,
! 2 int64, 3 real32, 4 real64), rank (int32), dims (int64 each), data.  The input file is written by
! tests/test_plan_relax.py, which replays the script on the numpy model and compares every record of the dump bit for
! bit, the return code of every call included: a code is recorded, never stopped on.
!
! The script: create, set_boundary(PERIODIC), import_device of all seven arrays - relax on the block (sl0, n), all
! tracers, to the horizontal mean (target null), with mean - relax on the whole plan, tracers [t1, t1+tn), to a given
! target, with mean (which must come back as the target) - run - export_device - destroy.
module relax_calls_hip
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
end module relax_calls_hip

program relax_calls
  use iso_c_binding
  use mpdata_grid
  use mpdata_hip_mod
  use relax_calls_hip
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
  real(rp), allocatable, target :: c_a(:,:), c_b(:,:), tgt_b(:,:,:), mean_a(:,:,:), mean_b(:,:,:)
  real(rp), allocatable, target :: fout(:,:,:,:), fluxout(:,:,:)
  type(c_ptr) :: d_f, d_u, d_w, d_rho, d_rhow, d_adz, d_flux, d_c, d_tgt, d_mean

  if (command_argument_count() < 2) error stop 'usage: relax_calls <input file> <dump file>'
  call get_command_argument(1, infile)
  call get_command_argument(2, outfile)
  open(unit=UIN, file=trim(infile), access='stream', form='unformatted', status='old')
  open(unit=UOUT, file=trim(outfile), access='stream', form='unformatted', status='replace')

  call get_i8('params', prm, [8])
  ncrms = prm(1); T = int(prm(4)); sl0 = prm(5); n = prm(6); t1 = int(prm(7)); tn = int(prm(8))
  call grid_set(ncrms, int(prm(2)), int(prm(3)), T)

  allocate(f(ncrms, -2:nx+3, nzm, T), u(ncrms, -1:nx+3, nzm), w(ncrms, -1:nx+2, nz), rho(ncrms, nzm), rhow(ncrms, nz), &
           flux(ncrms, nz, T))
  allocate(c_a(n, nzm), c_b(ncrms, nzm), tgt_b(ncrms, nzm, tn), mean_a(n, nzm, T), mean_b(ncrms, nzm, tn))
  allocate(fout(ncrms, -2:nx+3, nzm, T), fluxout(ncrms, nz, T))
  call get_r('f', f, shape(f));       call get_r('u', u, shape(u));          call get_r('w', w, shape(w))
  call get_r('rho', rho, shape(rho)); call get_r('rhow', rhow, shape(rhow)); call get_r('adz', adz, shape(adz))
  call get_r('flux', flux, shape(flux))
  call get_r('c_a', c_a, shape(c_a)); call get_r('c_b', c_b, shape(c_b)); call get_r('tgt_b', tgt_b, shape(tgt_b))
  close(UIN)

  call dalloc(d_f, size(f)); call dalloc(d_u, size(u)); call dalloc(d_w, size(w)); call dalloc(d_rho, size(rho))
  call dalloc(d_rhow, size(rhow)); call dalloc(d_adz, size(adz)); call dalloc(d_flux, size(flux))
  call dalloc(d_c, max(size(c_a), size(c_b))); call dalloc(d_tgt, size(tgt_b))
  call dalloc(d_mean, max(size(mean_a), size(mean_b)))

  ! ---- the plan, filled from device arrays
  call note(mpdata_set_variant(0_c_int), 'set_variant')
  plan = c_null_ptr
  call note(mpdata_plan_create_c(nslices, nx, nz, ntracers, plan), 'create')
  if (.not. c_associated(plan)) error stop 'no plan'
  call note(mpdata_plan_set_boundary_c(plan, MPDATA_BOUNDARY_PERIODIC), 'set_boundary')
  call to_dev(d_f, f, size(f)); call to_dev(d_u, u, size(u)); call to_dev(d_w, w, size(w)); call to_dev(d_rho, rho, size(rho))
  call to_dev(d_rhow, rhow, size(rhow)); call to_dev(d_adz, adz, size(adz)); call to_dev(d_flux, flux, size(flux))
  call note(mpdata_plan_import_device_c(plan, d_f, d_u, d_w, d_rho, d_rhow, d_adz, d_flux, 0_c_int, int(T, c_int)), 'import')

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
  call dfree(d_c); call dfree(d_tgt); call dfree(d_mean)
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

end program relax_calls
