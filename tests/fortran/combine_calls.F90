! combine_calls.F90 -- a TEST program: linear combinations of the tracers of a resident plan (include/mpdata_hip.h section
! 3z) driven from Fortran through the interfaces of mpdata_hip_mod alone.  It has no oracle and no interface block of its
! own for a library name.
!
!   ./combine_calls <input file> <dump file>       (combine_calls_sp: the -DMPDATA_SINGLE build, rp = c_float)
!
! Both files are streams of records in the format of calls_common.F90, which holds the helpers and the frame around the
! calls below as well (calls_open, calls_import, calls_close).  The input file is written by tests/test_plan_combine.py,
! which replays the script on the numpy model and compares every record of the dump bit for bit, the return code of every
! call included: a code is recorded, never stopped on.  Of `params`, t1 is a source tracer and tn the tracer dst here.
!
! The script: create, set_boundary(PERIODIC), import_device of all seven arrays - dst = coef1 * f(t1) + coef2 * f(dst) + c0 on
! the block (sl0, n), with sum - a clipped bit copy of dst into t1 on the whole plan (no coef, no c0, MPDATA_COMBINE_CLIP),
! with sum - the HOST form on the block: dst set to a profile (no source) - a call with MPDATA_COMBINE_MAX + 1 sources,
! which is refused - run - export_device - destroy.
program combine_calls
  use iso_c_binding
  use mpdata_grid
  use mpdata_hip_mod
  use calls_common
  implicit none
  real(rp), allocatable, target :: coef_a(:,:,:), c0_a(:,:), c0_c(:,:), sum_a(:,:), sum_b(:,:), sum_c(:,:)
  integer(c_int), target :: src_a(2), src_b(1), src_d(MPDATA_COMBINE_MAX + 1)
  type(c_ptr) :: d_coef, d_c0, d_sum

  call calls_open('combine_calls')
  allocate(coef_a(n, nzm, 2), c0_a(n, nzm), c0_c(n, nzm), sum_a(n, nzm), sum_b(ncrms, nzm), sum_c(n, nzm))
  call get_r('coef_a', coef_a, shape(coef_a)); call get_r('c0_a', c0_a, shape(c0_a)); call get_r('c0_c', c0_c, shape(c0_c))
  call dalloc(d_coef, size(coef_a)); call dalloc(d_c0, size(c0_a)); call dalloc(d_sum, size(sum_b))
  call calls_import()

  ! ---- the block: two sources, dst among them, coefficients, a level constant, with sum
  src_a = [int(t1, c_int), int(tn, c_int)]
  sum_a = SENTINEL
  call to_dev(d_coef, coef_a, size(coef_a)); call to_dev(d_c0, c0_a, size(c0_a)); call to_dev(d_sum, sum_a, size(sum_a))
  call note(mpdata_plan_combine_device_c(plan, sl0, n, int(tn, c_int), 2_c_int, c_loc(src_a), d_coef, d_c0, 0_c_int, d_sum), &
            'combine_block')
  call note(mpdata_plan_sync_c(plan), 'sync')
  call to_host(sum_a, d_sum, size(sum_a)); call put_r('sum_a', sum_a, shape(sum_a))

  ! ---- the whole plan: t1 = max(dst, 0), no multiply, nothing added
  src_b = [int(tn, c_int)]
  sum_b = SENTINEL
  call to_dev(d_sum, sum_b, size(sum_b))
  call note(mpdata_plan_combine_device_c(plan, 0_c_int64_t, ncrms, int(t1, c_int), 1_c_int, c_loc(src_b), c_null_ptr, c_null_ptr, &
                                         MPDATA_COMBINE_CLIP, d_sum), 'combine_clip')
  call note(mpdata_plan_sync_c(plan), 'sync')
  call to_host(sum_b, d_sum, size(sum_b)); call put_r('sum_b', sum_b, shape(sum_b))

  ! ---- the host form on the block: dst set to a profile
  sum_c = SENTINEL
#ifdef MPDATA_SINGLE
  call note(mpdata_plan_combine_f32_c(plan, sl0, n, int(tn, c_int), 0_c_int, c_null_ptr, c_null_ptr, c_loc(c0_c), 0_c_int, &
                                      c_loc(sum_c)), 'combine_set')
#else
  call note(mpdata_plan_combine_c(plan, sl0, n, int(tn, c_int), 0_c_int, c_null_ptr, c_null_ptr, c_loc(c0_c), 0_c_int, &
                                  c_loc(sum_c)), 'combine_set')
#endif
  call put_r('sum_c', sum_c, shape(sum_c))

  ! ---- refused: one source too many
  src_d = int(t1, c_int)
  call note(mpdata_plan_combine_device_c(plan, 0_c_int64_t, ncrms, int(tn, c_int), MPDATA_COMBINE_MAX + 1_c_int, c_loc(src_d), &
                                         c_null_ptr, c_null_ptr, 0_c_int, c_null_ptr), 'combine_many')

  call calls_close()
  call dfree(d_coef); call dfree(d_c0); call dfree(d_sum)
end program combine_calls
