! level_hist_calls.F90 -- a TEST program: the per-level histograms of a resident plan's tracers (include/mpdata_hip.h
! section 3ab) driven from Fortran through the interfaces of mpdata_hip_mod alone.  It has no oracle and no interface block
! of its own for a library name.
!
!   ./level_hist_calls <input file> <dump file>       (level_hist_calls_sp: the -DMPDATA_SINGLE build, rp = c_float)
!
! Both files are streams of records in the format of calls_common.F90, which holds the helpers and the frame around the
! calls below as well (calls_open, calls_import, calls_close).  The input file is written by tests/test_plan_level_hist.py,
! which replays the script on the numpy model and compares every record of the dump bit for bit, the return code of every
! call included: a code is recorded, never stopped on.  Of `params`, t1 is the binned tracer of the first and the third
! call and tn that of the second.  The edges arrive as records of the program's precision (the test draws them so) and are
! widened, exactly, to the real(c_double) HOST array every form takes.
!
! The script: create, set_boundary(PERIODIC), import_device of all seven arrays - on the block (sl0, n), tracer t1 in the 5
! bins of edges_a, cnt and bsum of all T tracers - on the whole plan, tracer tn in the 17 bins of edges_b, cnt alone - on the
! whole plan, tracer t1 in the 2 bins of edges_c, bsum of tracer tn alone - a call with 33 bins, which is refused - run -
! export_device (the call changed nothing) - destroy.
program level_hist_calls
  use iso_c_binding
  use mpdata_grid
  use mpdata_hip_mod
  use calls_common
  implicit none
  integer, parameter :: NA = 5, NBB = 17, NC = 2
  real(rp), allocatable :: ra(:), rb(:), rc_(:)
  real(c_double), allocatable, target :: edges_a(:), edges_b(:), edges_c(:)
  real(rp), allocatable, target :: cnt_a(:,:,:), bsum_a(:,:,:,:), cnt_b(:,:,:), bsum_c(:,:,:)
  type(c_ptr) :: d_cnt, d_bsum

  call calls_open('level_hist_calls')
  allocate(ra(NA + 1), rb(NBB + 1), rc_(NC + 1), edges_a(NA + 1), edges_b(NBB + 1), edges_c(NC + 1))
  allocate(cnt_a(n, nzm, NA), bsum_a(n, nzm, NA, T), cnt_b(ncrms, nzm, NBB), bsum_c(ncrms, nzm, NC))
  call get_r('edges_a', ra, shape(ra)); call get_r('edges_b', rb, shape(rb)); call get_r('edges_c', rc_, shape(rc_))
  edges_a = real(ra, c_double); edges_b = real(rb, c_double); edges_c = real(rc_, c_double)
  call dalloc(d_cnt, size(cnt_b)); call dalloc(d_bsum, max(size(bsum_a), size(bsum_c)))
  call calls_import()

  ! ---- the block, t1 in five bins, the counts and the sums of all tracers
  cnt_a = SENTINEL; bsum_a = SENTINEL
  call to_dev(d_cnt, cnt_a, size(cnt_a)); call to_dev(d_bsum, bsum_a, size(bsum_a))
  call note(mpdata_plan_level_hist_device_c(plan, sl0, n, int(t1, c_int), int(NA, c_int), c_loc(edges_a), d_cnt, d_bsum, 0_c_int, &
                                            int(T, c_int)), 'hist_block')
  call note(mpdata_plan_sync_c(plan), 'sync')
  call to_host(cnt_a, d_cnt, size(cnt_a)); call put_r('cnt_a', cnt_a, shape(cnt_a))
  call to_host(bsum_a, d_bsum, size(bsum_a)); call put_r('bsum_a', bsum_a, shape(bsum_a))

  ! ---- the whole plan, tn in seventeen bins, the counts alone (without bsum the tracer range is not looked at)
  cnt_b = SENTINEL
  call to_dev(d_cnt, cnt_b, size(cnt_b))
  call note(mpdata_plan_level_hist_device_c(plan, 0_c_int64_t, ncrms, int(tn, c_int), int(NBB, c_int), c_loc(edges_b), d_cnt, &
                                            c_null_ptr, int(T, c_int), 0_c_int), 'hist_cnt')
  call note(mpdata_plan_sync_c(plan), 'sync')
  call to_host(cnt_b, d_cnt, size(cnt_b)); call put_r('cnt_b', cnt_b, shape(cnt_b))

  ! ---- the whole plan, t1 in two bins, the sums of tracer tn alone
  bsum_c = SENTINEL
  call to_dev(d_bsum, bsum_c, size(bsum_c))
  call note(mpdata_plan_level_hist_device_c(plan, 0_c_int64_t, ncrms, int(t1, c_int), int(NC, c_int), c_loc(edges_c), c_null_ptr, &
                                            d_bsum, int(tn, c_int), 1_c_int), 'hist_sum')
  call note(mpdata_plan_sync_c(plan), 'sync')
  call to_host(bsum_c, d_bsum, size(bsum_c)); call put_r('bsum_c', bsum_c, shape(bsum_c))

  ! ---- refused: more bins than MPDATA_LEVEL_HIST_MAX_BINS
  call note(mpdata_plan_level_hist_device_c(plan, 0_c_int64_t, ncrms, int(t1, c_int), MPDATA_LEVEL_HIST_MAX_BINS + 1_c_int, &
                                            c_loc(edges_b), d_cnt, c_null_ptr, 0_c_int, 0_c_int), 'hist_refused')

  call calls_close()
  call dfree(d_cnt); call dfree(d_bsum)
end program level_hist_calls
