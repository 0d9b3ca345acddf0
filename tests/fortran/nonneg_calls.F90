! nonneg_calls.F90 -- a TEST program: the conservative per-level non-negativity fixer of a resident plan's tracers
! (include/mpdata_hip.h section 3x) driven from Fortran through the interfaces of mpdata_hip_mod alone.  It has no oracle
! and no interface block of its own for a library name.
!
!   ./nonneg_calls <input file> <dump file>       (nonneg_calls_sp: the -DMPDATA_SINGLE build, rp = c_float)
!
! Both files are streams of records in the format of calls_common.F90, which holds the helpers and the frame around the
! calls below as well (calls_open, calls_import, calls_close).  The input file is written by tests/test_plan_nonneg.py,
! which replays the script on the numpy model and compares every record of the dump bit for bit, the return code of every
! call included: a code is recorded, never stopped on.  The program has no input records of its own.
!
! The script: create, set_boundary(PERIODIC), import_device of all seven arrays - the device form on the block (sl0, n),
! all tracers, with sum and nneg - the device form on the whole plan, tracers [t1, t1+tn), with sum alone - the host form
! on the whole plan, with nneg alone (what the two calls before left to fix) - the array form on the block of the device
! array the plan was filled from, in place, with sum and nneg, and that array read back - a call with n = 0, which is
! refused - run - export_device - destroy.
! The host form and the array form of the program's precision: the module binds both precisions by their literal names.
#ifdef MPDATA_SINGLE
#define NONNEG_HOST mpdata_plan_nonneg_f32_c
#define NONNEG_ARRAY mpdata_nonneg_f32_device_c
#else
#define NONNEG_HOST mpdata_plan_nonneg_c
#define NONNEG_ARRAY mpdata_nonneg_device_c
#endif
program nonneg_calls
  use iso_c_binding
  use mpdata_grid
  use mpdata_hip_mod
  use calls_common
  implicit none
  real(rp), allocatable, target :: sum_a(:,:,:), nneg_a(:,:,:), sum_b(:,:,:), nneg_c(:,:,:), sum_d(:,:,:), nneg_d(:,:,:)
  type(c_ptr) :: d_sum, d_nneg

  call calls_open('nonneg_calls')
  allocate(sum_a(n, nzm, T), nneg_a(n, nzm, T), sum_b(ncrms, nzm, tn), nneg_c(ncrms, nzm, T), sum_d(n, nzm, T), nneg_d(n, nzm, T))
  call dalloc(d_sum, max(size(sum_a), size(sum_b))); call dalloc(d_nneg, size(nneg_a))
  call calls_import()

  ! ---- the device form: the block, all tracers, both outputs
  sum_a = SENTINEL; nneg_a = SENTINEL
  call to_dev(d_sum, sum_a, size(sum_a)); call to_dev(d_nneg, nneg_a, size(nneg_a))
  call note(mpdata_plan_nonneg_device_c(plan, sl0, n, d_sum, d_nneg, 0_c_int, int(T, c_int)), 'nonneg_block')
  call note(mpdata_plan_sync_c(plan), 'sync')
  call to_host(sum_a, d_sum, size(sum_a)); call put_r('sum_a', sum_a, shape(sum_a))
  call to_host(nneg_a, d_nneg, size(nneg_a)); call put_r('nneg_a', nneg_a, shape(nneg_a))

  ! ---- the device form: the whole plan, a tracer sub-range, the sum alone
  sum_b = SENTINEL
  call to_dev(d_sum, sum_b, size(sum_b))
  call note(mpdata_plan_nonneg_device_c(plan, 0_c_int64_t, ncrms, d_sum, c_null_ptr, int(t1, c_int), int(tn, c_int)), 'nonneg_range')
  call note(mpdata_plan_sync_c(plan), 'sync')
  call to_host(sum_b, d_sum, size(sum_b)); call put_r('sum_b', sum_b, shape(sum_b))

  ! ---- the host form: the whole plan, all tracers, the count alone
  nneg_c = SENTINEL
  call note(NONNEG_HOST(plan, 0_c_int64_t, ncrms, c_null_ptr, c_loc(nneg_c)), 'nonneg_host')
  call put_r('nneg_c', nneg_c, shape(nneg_c))

  ! ---- the array form: the block of the array the plan was filled from, in place
  sum_d = SENTINEL; nneg_d = SENTINEL
  call to_dev(d_sum, sum_d, size(sum_d)); call to_dev(d_nneg, nneg_d, size(nneg_d))
  call note(NONNEG_ARRAY(ncrms, nx, nz, int(T, c_int), sl0, n, d_f, d_sum, d_nneg, c_null_ptr), 'nonneg_array')
  call note(hipDeviceSynchronize(), 'dsync')
  call to_host(sum_d, d_sum, size(sum_d)); call put_r('sum_d', sum_d, shape(sum_d))
  call to_host(nneg_d, d_nneg, size(nneg_d)); call put_r('nneg_d', nneg_d, shape(nneg_d))
  call to_host(fout, d_f, size(fout)); call put_r('f_arr', fout, shape(fout))

  ! ---- refused: an empty block
  call note(mpdata_plan_nonneg_device_c(plan, sl0, 0_c_int64_t, d_sum, d_nneg, 0_c_int, int(T, c_int)), 'nonneg_none')

  call calls_close()
  call dfree(d_sum); call dfree(d_nneg)
end program nonneg_calls
