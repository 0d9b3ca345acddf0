! level_draft_calls.F90 -- a TEST program: the per-level updraft / downdraft sampling of a resident plan (include/mpdata_hip.h
! section 3ac) driven from Fortran through the interfaces of mpdata_hip_mod alone.  It has no oracle and no interface block
! of its own for a library name.
!
!   ./level_draft_calls <input file> <dump file>       (level_draft_calls_sp: the -DMPDATA_SINGLE build, rp = c_float)
!
! Both files are streams of records in the format of calls_common.F90, which holds the helpers and the frame around the
! calls below as well (calls_open, calls_import, calls_close).  The input file is written by tests/test_plan_level_draft.py,
! which replays the script on the numpy model and compares every record of the dump bit for bit, the return code of every
! call included: a code is recorded, never stopped on.  Of `params`, t1 is the condition tracer of the first call and tn
! that of the third.  The thresholds arrive as a record `thr` of two reals of the program's precision (wup, wdn) and are
! widened, exactly, to the real(c_double) values every form takes.
!
! The script: create, set_boundary(PERIODIC), import_device of all seven arrays - on the block (sl0, n), tracer t1 inside
! (lo_a, hi_a] against (wup, wdn), all four outputs of all T tracers - on the whole plan, no tracer condition (tc = -1), cnt
! and wsum alone with a tracer range that is not looked at - on the whole plan, tracer tn up to hi_c against (wup, -inf), wfsum
! of tracer t1 alone - a call with wdn > wup, which is refused - run - export_device (the call changed nothing) - destroy.
program level_draft_calls
  use iso_c_binding
  use, intrinsic :: ieee_arithmetic
  use mpdata_grid
  use mpdata_hip_mod
  use calls_common
  implicit none
  real(rp), allocatable, target :: thr(:), lo_a(:,:), hi_a(:,:), hi_c(:,:)
  real(rp), allocatable, target :: cnt_a(:,:,:), wsum_a(:,:,:), fsum_a(:,:,:,:), wfsum_a(:,:,:,:), cnt_b(:,:,:), wsum_b(:,:,:), wfsum_c(:,:,:)
  real(c_double) :: wup, wdn, ninf
  type(c_ptr) :: d_lo, d_hi, d_cnt, d_wsum, d_fsum, d_wfsum

  call calls_open('level_draft_calls')
  allocate(thr(2), lo_a(n, nzm), hi_a(n, nzm), hi_c(ncrms, nzm))
  allocate(cnt_a(n, nzm, 3), wsum_a(n, nzm, 3), fsum_a(n, nzm, 3, T), wfsum_a(n, nzm, 3, T))
  allocate(cnt_b(ncrms, nzm, 3), wsum_b(ncrms, nzm, 3), wfsum_c(ncrms, nzm, 3))
  call get_r('thr', thr, shape(thr))
  call get_r('lo_a', lo_a, shape(lo_a)); call get_r('hi_a', hi_a, shape(hi_a)); call get_r('hi_c', hi_c, shape(hi_c))
  wup = real(thr(1), c_double); wdn = real(thr(2), c_double)
  ninf = ieee_value(ninf, ieee_negative_inf)
  call dalloc(d_lo, size(hi_c)); call dalloc(d_hi, size(hi_c)); call dalloc(d_cnt, size(cnt_b)); call dalloc(d_wsum, size(wsum_b))
  call dalloc(d_fsum, int(ncrms) * nzm * 3 * T); call dalloc(d_wfsum, int(ncrms) * nzm * 3 * T)
  call calls_import()

  ! ---- the block, t1 inside (lo, hi], all four outputs of all tracers
  cnt_a = SENTINEL; wsum_a = SENTINEL; fsum_a = SENTINEL; wfsum_a = SENTINEL
  call to_dev(d_lo, lo_a, size(lo_a)); call to_dev(d_hi, hi_a, size(hi_a))
  call to_dev(d_cnt, cnt_a, size(cnt_a)); call to_dev(d_wsum, wsum_a, size(wsum_a))
  call to_dev(d_fsum, fsum_a, size(fsum_a)); call to_dev(d_wfsum, wfsum_a, size(wfsum_a))
  call note(mpdata_plan_level_draft_device_c(plan, sl0, n, int(t1, c_int), d_lo, d_hi, wup, wdn, d_cnt, d_wsum, d_fsum, d_wfsum, &
                                             0_c_int, int(T, c_int)), 'draft_block')
  call note(mpdata_plan_sync_c(plan), 'sync')
  call to_host(cnt_a, d_cnt, size(cnt_a)); call put_r('cnt_a', cnt_a, shape(cnt_a))
  call to_host(wsum_a, d_wsum, size(wsum_a)); call put_r('wsum_a', wsum_a, shape(wsum_a))
  call to_host(fsum_a, d_fsum, size(fsum_a)); call put_r('fsum_a', fsum_a, shape(fsum_a))
  call to_host(wfsum_a, d_wfsum, size(wfsum_a)); call put_r('wfsum_a', wfsum_a, shape(wfsum_a))

  ! ---- the whole plan, no tracer condition, cnt and wsum alone (without fsum and wfsum the tracer range is not looked at)
  cnt_b = SENTINEL; wsum_b = SENTINEL
  call to_dev(d_cnt, cnt_b, size(cnt_b)); call to_dev(d_wsum, wsum_b, size(wsum_b))
  call note(mpdata_plan_level_draft_device_c(plan, 0_c_int64_t, ncrms, -1_c_int, c_null_ptr, c_null_ptr, wup, wdn, d_cnt, d_wsum, &
                                             c_null_ptr, c_null_ptr, int(T, c_int), 0_c_int), 'draft_w')
  call note(mpdata_plan_sync_c(plan), 'sync')
  call to_host(cnt_b, d_cnt, size(cnt_b)); call put_r('cnt_b', cnt_b, shape(cnt_b))
  call to_host(wsum_b, d_wsum, size(wsum_b)); call put_r('wsum_b', wsum_b, shape(wsum_b))

  ! ---- the whole plan, tn up to hi, no downdraft class (wdn = -inf), wfsum of tracer t1 alone
  wfsum_c = SENTINEL
  call to_dev(d_hi, hi_c, size(hi_c)); call to_dev(d_wfsum, wfsum_c, size(wfsum_c))
  call note(mpdata_plan_level_draft_device_c(plan, 0_c_int64_t, ncrms, int(tn, c_int), c_null_ptr, d_hi, wup, ninf, c_null_ptr, &
                                             c_null_ptr, c_null_ptr, d_wfsum, int(t1, c_int), 1_c_int), 'draft_up')
  call note(mpdata_plan_sync_c(plan), 'sync')
  call to_host(wfsum_c, d_wfsum, size(wfsum_c)); call put_r('wfsum_c', wfsum_c, shape(wfsum_c))

  ! ---- refused: wdn > wup
  call note(mpdata_plan_level_draft_device_c(plan, 0_c_int64_t, ncrms, int(t1, c_int), c_null_ptr, c_null_ptr, wdn, wup, d_cnt, &
                                             c_null_ptr, c_null_ptr, c_null_ptr, 0_c_int, 0_c_int), 'draft_refused')

  call calls_close()
  call dfree(d_lo); call dfree(d_hi); call dfree(d_cnt); call dfree(d_wsum); call dfree(d_fsum); call dfree(d_wfsum)
end program level_draft_calls
