! level_cond_calls.F90 -- a TEST program: the per-level conditional counts and sums of a resident plan's tracers
! (include/mpdata_hip.h section 3v) driven from Fortran through the interfaces of mpdata_hip_mod alone.  It has no oracle
! and no interface block of its own for a library name.
!
!   ./level_cond_calls <input file> <dump file>       (level_cond_calls_sp: the -DMPDATA_SINGLE build, rp = c_float)
!
! Both files are streams of records in the format of calls_common.F90, which holds the helpers and the frame around the
! calls below as well (calls_open, calls_import, calls_close).  The input file is written by tests/test_plan_level_cond.py,
! which replays the script on the numpy model and compares every record of the dump bit for bit, the return code of every
! call included: a code is recorded, never stopped on.  Of `params`, t1 is the condition tracer of the first and the third
! call and tn that of the second.
!
! The script: create, set_boundary(PERIODIC), import_device of all seven arrays - on the block (sl0, n), tracer t1 inside
! (lo_a, hi_a], cnt and csum of all T tracers - on the whole plan, tracer tn above lo_b, cnt alone - on the whole plan,
! tracer t1 up to hi_c, csum of tracer tn alone - a call without a bound, which is refused - run - export_device (the call
! changed nothing) - destroy.
program level_cond_calls
  use iso_c_binding
  use mpdata_grid
  use mpdata_hip_mod
  use calls_common
  implicit none
  real(rp), allocatable, target :: lo_a(:,:), hi_a(:,:), lo_b(:,:), hi_c(:,:), cnt_a(:,:), csum_a(:,:,:), cnt_b(:,:), csum_c(:,:)
  type(c_ptr) :: d_lo, d_hi, d_cnt, d_csum

  call calls_open('level_cond_calls')
  allocate(lo_a(n, nzm), hi_a(n, nzm), lo_b(ncrms, nzm), hi_c(ncrms, nzm), cnt_a(n, nzm), csum_a(n, nzm, T), cnt_b(ncrms, nzm), &
           csum_c(ncrms, nzm))
  call get_r('lo_a', lo_a, shape(lo_a)); call get_r('hi_a', hi_a, shape(hi_a))
  call get_r('lo_b', lo_b, shape(lo_b)); call get_r('hi_c', hi_c, shape(hi_c))
  call dalloc(d_lo, size(lo_b)); call dalloc(d_hi, size(hi_c)); call dalloc(d_cnt, size(cnt_b))
  call dalloc(d_csum, int(ncrms) * nzm * T)
  call calls_import()

  ! ---- the block, t1 inside (lo, hi], the count and the sums of all tracers
  cnt_a = SENTINEL; csum_a = SENTINEL
  call to_dev(d_lo, lo_a, size(lo_a)); call to_dev(d_hi, hi_a, size(hi_a))
  call to_dev(d_cnt, cnt_a, size(cnt_a)); call to_dev(d_csum, csum_a, size(csum_a))
  call note(mpdata_plan_level_cond_device_c(plan, sl0, n, int(t1, c_int), d_lo, d_hi, d_cnt, d_csum, 0_c_int, int(T, c_int)), &
            'cond_block')
  call note(mpdata_plan_sync_c(plan), 'sync')
  call to_host(cnt_a, d_cnt, size(cnt_a)); call put_r('cnt_a', cnt_a, shape(cnt_a))
  call to_host(csum_a, d_csum, size(csum_a)); call put_r('csum_a', csum_a, shape(csum_a))

  ! ---- the whole plan, tn above lo, the count alone (without csum the tracer range is not looked at)
  cnt_b = SENTINEL
  call to_dev(d_lo, lo_b, size(lo_b)); call to_dev(d_cnt, cnt_b, size(cnt_b))
  call note(mpdata_plan_level_cond_device_c(plan, 0_c_int64_t, ncrms, int(tn, c_int), d_lo, c_null_ptr, d_cnt, c_null_ptr, &
                                            int(T, c_int), 0_c_int), 'cond_lo')
  call note(mpdata_plan_sync_c(plan), 'sync')
  call to_host(cnt_b, d_cnt, size(cnt_b)); call put_r('cnt_b', cnt_b, shape(cnt_b))

  ! ---- the whole plan, t1 up to hi, the sum of tracer tn alone
  csum_c = SENTINEL
  call to_dev(d_hi, hi_c, size(hi_c)); call to_dev(d_csum, csum_c, size(csum_c))
  call note(mpdata_plan_level_cond_device_c(plan, 0_c_int64_t, ncrms, int(t1, c_int), c_null_ptr, d_hi, c_null_ptr, d_csum, &
                                            int(tn, c_int), 1_c_int), 'cond_hi')
  call note(mpdata_plan_sync_c(plan), 'sync')
  call to_host(csum_c, d_csum, size(csum_c)); call put_r('csum_c', csum_c, shape(csum_c))

  ! ---- refused: no bound at all
  call note(mpdata_plan_level_cond_device_c(plan, 0_c_int64_t, ncrms, int(t1, c_int), c_null_ptr, c_null_ptr, d_cnt, d_csum, &
                                            0_c_int, int(T, c_int)), 'cond_refused')

  call calls_close()
  call dfree(d_lo); call dfree(d_hi); call dfree(d_cnt); call dfree(d_csum)
end program level_cond_calls
