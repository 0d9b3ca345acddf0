"""GPU tests of the running column integrals of a resident plan (include/mpdata_hip.h 3aa):
mpdata_plan_column_scan_device, the host forms, the array forms, their Python face Plan.column_scan / column_scan_host /
column_scan, and the Fortran program tests/fortran/column_scan_calls.F90.

Every comparison is bit for bit (util.assert_bitwise) against the numpy model of tests/column_scan_model.py: CS.column_scan
on a reference-layout truth, or the plan model with the new call (CS.PlanModelColumnScan: an EXACT plan's f and flux are
bit-identical to it), or, for FAST plans, the plan's own whole export before the call.  The whole export of f -- every
tracer, the halos -- AND flux is compared after each call.  wgt lies inside a larger buffer with 4 KiB of NaN on both
sides, so a read outside the block's array poisons the result, and must come back unchanged; total is filled with NaN and
lies between two bands of 4 KiB of NaN as well, which must come back unchanged bit for bit.  wgt is signed, of magnitude 0.25 .. 1; f is the
oracle's raw field moved by one half, so signed.  u and w have no export: that they keep their bits shows in the run behind
the calls, which is compared with the model's.

Shapes (ncrms, nx, nz): those of tests/test_plan_vsolve.py, the smallest at which the staging kernel takes another path (G =
16 adjacent 8-byte elements of the instance axis a workgroup owns, fewer where the levels do not fit; a column batch with
a remainder at nx = 11; one, two and three 64-element slices of a chunk and a tail wave), every one with three tracers so
that dst lies below, above and on src."""
import numpy as np
import pytest

import column_scan_model as CS
import fortran_records as FR
import plan_harness as H
from oracle import plan_model as PM
from plan_harness import BAND, _defaults, nan_banded, nan_out, upload
from util import assert_bitwise, to_dev, to_host

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
G = 16
T = 3

# name -> (shape, tracers, dtype, switches)
KINDS = {
    "f64-nz3": ((5, 11, 3), T, F64, {}),
    "f64-nz28": ((5, 1, 28), T, F64, {}), "f64-nz28-3groups": ((2 * G + 5, 11, 28), T, F64, {}),
    "f64-nz34": ((5, 11, 34), T, F64, {}), "f64-nz65": ((5, 1, 65), T, F64, {}), "f64-nz66": ((5, 11, 66), T, F64, {}),
    "f64-nz72": ((5, 3, 72), T, F64, {}), "f64-nz130": ((5, 1, 130), T, F64, {}), "f64-nz238": ((5, 11, 238), T, F64, {}),
    "f32-nz28-even": ((6, 11, 28), T, F32, {}), "f32-nz28-3groups": ((4 * G + 10, 1, 28), T, F32, {}),
    "f32-nz72-even": ((6, 3, 72), T, F32, {}),
    "f32-nz28-odd": ((2 * G + 5, 11, 28), T, F32, dict(odd=True)), "f32-nz72-odd": ((5, 1, 72), T, F32, dict(odd=True)),
    "f32-nz3-odd": ((5, 3, 3), T, F32, dict(odd=True)),
    "f64-nz12-ref": ((5, 3, 12), T, F64, dict(ref=True)),
    "f32-nz28-odd-ref": ((5, 3, 28), T, F32, {}),      # (an odd fp32 plan without the switch keeps the reference layout)
    "f64-nz239-tall": ((5, 3, 239), T, F64, dict(tall=True)), "f64-nz300-tall": ((5, 1, 300), T, F64, dict(tall=True)),
    "f64-nz239-tall-3groups": ((2 * G + 5, 1, 239), T, F64, dict(tall=True)),
    "f32-nz250-tall": ((6, 3, 250), T, F32, dict(tall=True)),
    "f32-nz239-tall-odd": ((5, 2, 239), T, F32, dict(tall=True, odd=True)),
}
REF = ("f64-nz12-ref", "f32-nz28-odd-ref")
# one kind of each family runs the FAST variant too; one of each a PERIODIC plan
FAST = ("f64-nz28-3groups", "f64-nz72", "f32-nz28-odd", "f64-nz12-ref", "f64-nz239-tall")
PERIODIC = ("f64-nz34", "f32-nz72-odd", "f64-nz12-ref", "f32-nz239-tall-odd", "f64-nz300-tall")
SEED = 100
UP, DOWN, EXCL = 0, CS.DOWN, CS.EXCLUSIVE

# pass A, no run between: (src, dst, wgt given, mode, total) -- all four modes, dst above, below and on src, wgt given and
# NULL, total on and off
SCRIPT = ((0, 2, True, UP, True), (2, 0, False, DOWN, True), (1, 1, True, EXCL, False), (2, 1, False, DOWN | EXCL, True),
          (0, 0, False, UP, True), (1, 2, True, DOWN, False), (2, 2, True, DOWN | EXCL, True), (1, 0, False, EXCL, True))
# pass B, with a run behind each (the second call stands behind a run: a windowed plan's seams are stale)
RSCRIPT = ((1, 0, True, DOWN, True), (2, 2, False, UP | EXCL, True), (0, 1, False, DOWN | EXCL, False), (2, 1, True, UP, True))
# periodic: (k, src, dst, wgt given, mode)
PSCRIPT = ((5, 0, 2, True, DOWN), (6, 2, 2, False, EXCL), (7, 1, 0, True, UP), (8, 0, 1, False, DOWN | EXCL))

_INPUTS = {}


def inputs(oracle, name):
    """the seven arrays of KINDS[name]: computed once and shared; no test writes them"""
    if name not in _INPUTS:
        shape, ntr, dt, _ = KINDS[name]
        _INPUTS[name] = CS.make_plan_inputs(oracle, shape, ntr, dt, SEED)
    return _INPUTS[name]


def new_plan(M, name, variant=None):
    return H.new_plan(M, KINDS[name], name, name in REF, bool(KINDS[name][3].get("tall")), variant)


def model_of(oracle, name):
    shape, ntr, dt, _ = KINDS[name]
    m = CS.PlanModelColumnScan(oracle, *shape, ntr, dt)
    assert m.upload({k: np.array(v, order="F") for k, v in inputs(oracle, name).items()}) is None
    return m


def whole(M, p, name, what=("f", "flux")):
    return H.whole(M, p, KINDS[name], what)


def same_as_model(M, p, name, m, what):
    H.same_as_model(M, p, KINDS[name], name, m, what)


def wgt_of(name, k, given, sl0=0, n=None):
    shape, _, dt, _ = KINDS[name]
    n = shape[0] - sl0 if n is None else n
    return CS.make_wgt(n, shape[2], dt, 500 + k) if given else None


def nan_total(shape, dt):
    """(raw, pristine copy, view of torch `shape`): a buffer of NaN, the view between two bands of BAND bytes of it"""
    import torch
    numel = int(np.prod(shape))
    pad = BAND // np.dtype(dt).itemsize
    raw = torch.full((numel + 2 * pad,), float("nan"), dtype=H.tdt(dt), device="cuda:0")
    return raw, raw.clone(), raw[pad:pad + numel].view(tuple(shape))


def total_bands_kept(raw, pristine, dt):
    import torch
    pad = BAND // np.dtype(dt).itemsize
    u = torch.int64 if np.dtype(dt).itemsize == 8 else torch.int32
    return torch.equal(raw[:pad].view(u), pristine[:pad].view(u)) and torch.equal(raw[-pad:].view(u), pristine[-pad:].view(u))


def scan(M, p, name, src, dst, wgt=None, mode=0, sl0=0, n=None, total=True, call=None):
    """Plan.column_scan of host wgt (n, nzm) or None -> total (n, nx) or None; wgt and the bands are checked.  call: another
    callable with Plan.column_scan's arguments (a shard plan's)."""
    import torch
    shape, _, dt, _ = KINDS[name]
    nx, nz = shape[1], shape[2]
    n = shape[0] - sl0 if n is None else n
    assert wgt is None or (wgt.shape == (n, nz - 1) and wgt.dtype == dt)
    sh = M.column_scan_shapes(n, nx, nz)
    win = nan_banded(wgt, sh["wgt"]) if wgt is not None else None
    orig = win[0].clone() if win else None
    buf = nan_total(sh["total"], dt) if total else None
    torch.cuda.synchronize()      # (the plan may run on a stream that does not wait for the one that filled the buffers)
    (call or p.column_scan)(src, dst, win[1] if win else None, buf[2] if buf else None, mode, sl0, n)
    p.sync()
    torch.cuda.synchronize()
    if win:
        assert torch.equal(win[0].view(torch.uint8), orig.view(torch.uint8)), "wgt changed"
    if not buf:
        return None
    raw, pristine, out = buf
    assert total_bands_kept(raw, pristine, dt), "total: a band byte changed"
    return to_host(out).reshape((n, nx), order="F")


def model_scan(m, src, dst, wgt=None, mode=0, sl0=0, n=None):
    t = m.column_scan(src, dst, wgt, mode, sl0=sl0, n=n)
    assert not isinstance(t, int), t
    return t


def step(M, p, m, name, k, src, dst, given, mode, total, what, sl0=0, n=None):
    """one call on the plan and the model: total and the whole plan compared"""
    w = wgt_of(name, k, given, sl0, n)
    want = model_scan(m, src, dst, w, mode, sl0, n)
    got = scan(M, p, name, src, dst, w, mode, sl0, n, total=total)
    if total:
        assert_bitwise(got, want, what + ": total")
    same_as_model(M, p, name, m, what)


# ---- 1. every kind of plan: whole plan, all four modes, every state
@pytest.mark.parametrize("name", list(KINDS))
def test_every_plan_kind(mpdata, oracle, name):
    M = mpdata
    shape, ntr, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    inp = inputs(oracle, name)
    F0 = inp["f"]
    assert (F0 < 0).any() and (F0 > 0).any()
    p = new_plan(M, name)
    upload(p, inp)
    m = model_of(oracle, name)
    # ---- pass A: behind the upload, call after call
    first = None
    for k, (src, dst, given, mode, total) in enumerate(SCRIPT):
        before = np.array(m.a["f"], order="F")
        step(M, p, m, name, k, src, dst, given, mode, total, f"{name} script {k} (src {src}, dst {dst}, wgt {given}, mode {mode})")
        after = m.a["f"]
        assert_bitwise(after[:, :3], before[:, :3], "the halos stay") or assert_bitwise(after[:, nx + 3:], before[:, nx + 3:], "the halos stay")
        for t in range(ntr):
            if t != dst:
                assert_bitwise(after[..., t], before[..., t], f"tracer {t} stays")
        assert not np.array_equal(after[..., dst], before[..., dst]), k
        if k == 0:
            first = np.array(after, order="F")
    # ---- pass B: the uploaded field again, a run behind every call
    upload(p, inp)
    m = model_of(oracle, name)
    for k, (src, dst, given, mode, total) in enumerate(RSCRIPT):
        what = f"{name} run script {k} (src {src}, dst {dst}, wgt {given}, mode {mode})"
        step(M, p, m, name, 20 + k, src, dst, given, mode, total, what)
        # a run on the kept velocities = export -> model -> import -> run: seams and the phantom are consistent
        p.run()
        assert m.run() is None
        same_as_model(M, p, name, m, what + ", run")
    if name in PERIODIC:
        assert m.set_boundary(PM.PERIODIC) is None
        p.set_boundary(M.BOUNDARY_PERIODIC)
        p.run()
        assert m.run() is None
        # (5) the halos are stale behind the run; the export hands out wrapped halos of the NEW dst
        # (6) on halos the export just wrapped: those of dst are copies of the OLD field now, the next export wraps again
        # (7) a run right behind the call, no read-back between   (8) back to GIVEN behind a call: the plan holds what an
        # export just before the switch would have returned
        for k, src, dst, given, mode in PSCRIPT:
            w = wgt_of(name, k, given)
            want = model_scan(m, src, dst, w, mode)
            got = scan(M, p, name, src, dst, w, mode, total=k != 7)
            if got is not None:
                assert_bitwise(got, want, f"{name} periodic {k}: total")
            if k == 7:
                p.run()
                assert m.run() is None
            if k == 8:
                p.set_boundary(M.BOUNDARY_GIVEN)
                assert m.set_boundary(PM.GIVEN) is None
            same_as_model(M, p, name, m, f"periodic {k}")
            if k in (5, 6):
                e = whole(M, p, name, ("f",))["f"]
                assert_bitwise(e, PM.wrap(np.array(e, order="F")), f"{name} periodic {k}: the halos are wrapped copies of the new interior")
    p.close()
    if name in FAST:
        # FAST: the same bits as EXACT on the uploaded f; after a run against the plan's own export changed by the model
        p = new_plan(M, name, variant=M.VARIANT_FAST)
        upload(p, inp)
        src, dst, given, mode, _ = SCRIPT[0]
        scan(M, p, name, src, dst, wgt_of(name, 0, given), mode)
        assert_bitwise(whole(M, p, name, ("f",))["f"], first, f"{name} FAST upload, scan")
        upload(p, inp)
        p.run()
        wra = CS.weights(inp["rho"], inp["adz"])
        for k, (src, dst, given, mode, _) in enumerate(RSCRIPT):
            E = whole(M, p, name, ("f",))["f"]
            w = wgt_of(name, 30 + k, given)
            got = scan(M, p, name, src, dst, w, mode)
            want_E, t_E = CS.column_scan(E, src, dst, wra if w is None else w, mode)
            assert_bitwise(got, t_E, f"{name} FAST run, scan {k}: total")
            assert_bitwise(whole(M, p, name, ("f",))["f"], want_E, f"{name} FAST run, scan {k}")
        p.close()


# ---- 2. blocks: what lies outside keeps every bit (the block lists of tests/test_plan_vsolve.py)
BLOCKS = {
    # two per tile, five instances: inside one group, one instance, the last one
    "f64-nz28": [(1, 3), (2, 1), (4, 1), (0, 5)],
    # three groups: a block that straddles a group boundary, odd sl0 across two boundaries, the last instance alone, a group
    "f64-nz28-3groups": [(G - 1, 3), (3, 2 * G), (2 * G + 4, 1), (G, G)],
    "f64-nz72": [(1, 1), (1, 2)],
    "f64-nz130": [(1, 1), (0, 1)],
    # fp32 pairs: odd sl0 and odd n (split pairs at both ends), one half, a whole pair
    "f32-nz28-even": [(1, 3), (5, 1), (2, 2)],
    # 37 pairs: across a group boundary (2G instances per group), splitting pairs
    "f32-nz28-3groups": [(2 * G - 1, 3), (1, 4 * G + 4), (4 * G + 9, 1)],
    # fp32 pairs, odd plan of 37 (instance 36 shares its pair with the phantom): blocks that hold and miss instance 36
    "f32-nz28-odd": [(1, 2), (36, 1), (35, 2), (0, 36), (33, 3), (0, 37)],
    "f32-nz72-odd": [(4, 1), (1, 1), (0, 2), (3, 2)],
    "f32-nz28-odd-ref": [(1, 3), (4, 1)],
    "f64-nz12-ref": [(1, 3), (4, 1)],
    # windowed plans: each behind an import (the first) and behind a run (the others: stale seams), a block and the whole
    "f64-nz239-tall": [(1, 1), (0, 1), (0, 2), (2, 3)],
    "f64-nz239-tall-3groups": [(G - 1, 3), (2 * G + 4, 1), (1, 2 * G)],
    "f32-nz239-tall-odd": [(1, 1), (4, 1), (0, 2), (3, 2), (0, 5)],
    "f32-nz250-tall": [(1, 3), (5, 1)],
}
# the calls rotate: (src, dst, wgt given, mode, total)
BCALLS = ((0, 2, True, DOWN, True), (1, 1, False, UP, True), (2, 0, True, DOWN | EXCL, False), (1, 2, False, EXCL, True),
          (0, 0, True, DOWN, True), (2, 1, False, UP, True))


@pytest.mark.parametrize("name", list(BLOCKS))
def test_blocks_leave_the_rest_alone(mpdata, oracle, name):
    M = mpdata
    shape, ntr, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    p = new_plan(M, name)
    upload(p, inputs(oracle, name))
    m = model_of(oracle, name)
    for k, (sl0, n) in enumerate(BLOCKS[name]):
        src, dst, given, mode, total = BCALLS[k % len(BCALLS)]
        what = f"{name} block {sl0, n} src {src} dst {dst} mode {mode}"
        before = whole(M, p, name)
        w = wgt_of(name, 10 + k, given, sl0, n)
        want_t = model_scan(m, src, dst, w, mode, sl0, n)
        got = scan(M, p, name, src, dst, w, mode, sl0, n, total=total)
        if total:
            assert_bitwise(got, want_t, what + ": total")
        after = whole(M, p, name)
        out = np.ones(ncrms, bool)
        out[sl0:sl0 + n] = False
        assert_bitwise(after["f"][out], before["f"][out], what + ": instances outside")
        for t in range(ntr):
            if t != dst:
                assert_bitwise(after["f"][..., t], before["f"][..., t], what + f": tracer {t}")
        assert_bitwise(after["flux"], before["flux"], what + ": flux")
        b = slice(sl0, sl0 + n)
        inp = inputs(oracle, name)
        want = CS.column_scan(before["f"][b], src, dst, CS.weights(inp["rho"][b], inp["adz"][b]) if w is None else w, mode)[0]
        assert_bitwise(after["f"][b], want, what + ": inside")
        assert not np.array_equal(want[..., dst], before["f"][b][..., dst])
        same_as_model(M, p, name, m, what)
        # a run of every instance (the phantom of an odd plan rides with instance ncrms - 1; a windowed plan refreshes
        # the seams the call marked stale; u, w, rho, rhow, adz enter it) matches the model
        p.run()
        assert m.run() is None
        same_as_model(M, p, name, m, what + ", run")
    p.close()


# ---- 3. cross-checks against the calls the plan already has
@pytest.mark.parametrize("name", ["f64-nz28-3groups", "f32-nz28-odd", "f64-nz12-ref", "f64-nz239-tall", "f32-nz250-tall", "f64-nz72"])
def test_cross_checks_against_existing_calls(mpdata, oracle, name):
    """UP total without wgt is Plan.column_path's path, in either inclusion mode, and so is level nzm of the inclusive UP
    scan; combine(dst, (src,)) followed by the scan of dst in place is the scan of src into dst"""
    M = mpdata
    shape, ntr, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    inp = inputs(oracle, name)
    p, q = new_plan(M, name), new_plan(M, name)
    upload(p, inp)
    upload(q, inp)
    path = nan_out(M.column_path_shapes(ncrms, nx, ntr)["path"], dt)
    p.column_path(path[2], None, 0, ncrms, 0, ntr)
    p.sync()
    path = to_host(path[2]).reshape((ncrms, nx, ntr), order="F")
    assert np.isfinite(path).all() and path.any()
    for k, (src, dst, mode) in enumerate(((0, 2, UP), (1, 1, EXCL), (2, 0, UP))):
        want = path[:, :, src] if src != 2 else None          # (tracer 2 was rewritten by the first call)
        tot = scan(M, p, name, src, dst, None, mode)
        if want is not None:
            assert_bitwise(tot, want, f"{name}: UP total of tracer {src} is column_path's path (mode {mode})")
        if mode == UP:
            e = whole(M, p, name, ("f",))["f"]
            assert_bitwise(e[:, 3:nx + 3, nz - 2, dst], tot, f"{name}: level nzm of the inclusive UP scan is total")
    # the two-tracer scan against the copy and the in-place scan, on the plan q
    r = new_plan(M, name)
    upload(r, inp)
    for k, mode in enumerate(CS.MODES):
        w = wgt_of(name, 60 + k, k % 2 == 0)
        src, dst = ((0, 1), (2, 0), (1, 2), (0, 2))[k]
        t2 = scan(M, q, name, src, dst, w, mode)
        r.combine(dst, (src,))
        t1 = scan(M, r, name, dst, dst, w, mode)
        assert_bitwise(t1, t2, f"{name} mode {mode}: total")
        eq, er = whole(M, q, name), whole(M, r, name)
        for key in eq:
            assert_bitwise(er[key], eq[key], f"{name} mode {mode}: copy + in-place scan == two-tracer scan: {key}")
    assert not np.array_equal(eq["f"], inp["f"])
    for x in (p, q, r):
        x.close()


# ---- 4. the host form and the array forms
@pytest.mark.parametrize("name", ["f64-nz28-3groups", "f32-nz28-odd", "f64-nz12-ref", "f64-nz72", "f64-nz239-tall", "f32-nz250-tall"])
def test_host_form(mpdata, oracle, name):
    M = mpdata
    shape, ntr, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    # (sl0, n, src, dst, wgt given, mode, total)
    script = ((0, ncrms, 0, 2, True, DOWN, True), (1, 1, 1, 1, False, EXCL, True), (ncrms - 1, 1, 2, 0, True, UP, False),
              (0, 2, 0, 1, False, DOWN | EXCL, True))
    p = new_plan(M, name)
    upload(p, inputs(oracle, name))
    m = model_of(oracle, name)
    for k, (sl0, n, src, dst, given, mode, total) in enumerate(script):
        w = wgt_of(name, 20 + k, given, sl0, n)
        keep = None if w is None else np.array(w, order="F")
        th = np.full((n, nx), np.nan, dt, order="F") if total else None
        p.column_scan_host(src, dst, w, th, mode, sl0, n)
        if w is not None:
            assert_bitwise(w, keep, f"{name} host {sl0, n}: wgt")
        want = model_scan(m, src, dst, w, mode, sl0, n)
        if total:
            assert_bitwise(th, want, f"{name} host {sl0, n}: total")
        same_as_model(M, p, name, m, f"host form {sl0, n}")
        p.run()
        assert m.run() is None
        same_as_model(M, p, name, m, f"host form {sl0, n}, run")
    with pytest.raises(M.MpdataError):
        p.column_scan_host(0, 1, CS.make_wgt(2, nz, dt, 1)[:, :-1], sl0=0, n=2)       # a wrong shape
    p.close()


# 257 and 600 instances: more than one block of 256 threads and a partly filled last one; (2, 70000, 3): the second trip
# over gridDim.y (the columns).  f and wgt are random, so instance b differs from b - 256 and column i from i - 65535.  Each
# with a block inside the arrays (sl0 > 0); f lies between NaN bands that must come back unchanged.  (5, 1, 2): one level,
# which no plan can have.
ARRAYS = {"nz2": ((5, 1, 2), (1, 3)), "n257": ((257, 3, 6), (1, 256)), "n600": ((600, 2, 5), (300, 299)), "cols70000": ((2, 70000, 3), (1, 1))}


@pytest.mark.parametrize("case", list(ARRAYS))
@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
def test_array_forms(mpdata, dt, case):
    import torch
    M = mpdata
    (ncrms, nx, nz), (b0, bn) = ARRAYS[case]
    rng = np.random.default_rng([77, ncrms, nx])
    f = np.asfortranarray(rng.uniform(-0.5, 0.5, (ncrms, nx + 6, nz - 1, T)).astype(dt))
    calls = (((0, ncrms), 0, 2, UP), ((b0, bn), 2, 0, DOWN | EXCL), ((b0, bn), 1, 1, DOWN), ((0, ncrms), 1, 2, EXCL))
    for (sl0, n), src, dst, mode in calls:
        w = CS.make_wgt(n, nz, dt, 600 + sl0 + mode)
        want, want_t = CS.column_scan(f[sl0:sl0 + n], src, dst, w, mode)
        full = np.array(f, order="F")
        full[sl0:sl0 + n] = want
        if n > 256:
            assert not np.array_equal(want[256:], want[:n - 256]) and not np.array_equal(want_t[256:], want_t[:n - 256])
        if nx > 65535:
            assert not np.array_equal(want_t[:, 65535:], want_t[:, :nx - 65535])
        fraw, fd = nan_banded(f, (T, nz - 1, nx + 6, ncrms))
        pad = (fraw.numel() - fd.numel()) // 2
        sh = M.column_scan_shapes(n, nx, nz)
        wraw, wv = nan_banded(w, sh["wgt"])
        worig = wraw.clone()
        bd = nan_total(sh["total"], dt)
        torch.cuda.synchronize()
        M.column_scan(fd, src, dst, wv, bd[2], mode, sl0, n)
        torch.cuda.synchronize()
        assert torch.isnan(fraw[:pad]).all() and torch.isnan(fraw[-pad:]).all(), "a guard band of f changed"
        assert total_bands_kept(bd[0], bd[1], dt) and torch.equal(wraw.view(torch.uint8), worig.view(torch.uint8))
        assert_bitwise(to_host(fd), full, f"array form {case} block {sl0, n} src {src} dst {dst} mode {mode}: f")
        assert_bitwise(to_host(bd[2]).reshape((n, nx), order="F"), want_t, f"array form {case} block {sl0, n}: total")
        f = full
    # total skipped
    fd = to_dev(f)
    w = CS.make_wgt(ncrms, nz, dt, 650)
    M.column_scan(fd, 0, 1, to_dev(w))
    torch.cuda.synchronize()
    assert_bitwise(to_host(fd), CS.column_scan(f, 0, 1, w)[0], f"array form {case}, without total: f")


# ---- 5. every error code, in the stated order; the plan's state before and after
def test_errors_change_nothing(mpdata, oracle):
    M = mpdata
    name = "f64-nz72"
    shape, ntr, dt, _ = KINDS[name]
    ncrms, nx, nz = shape
    inp = inputs(oracle, name)

    def code(fn, *a, **kw):
        with pytest.raises(M.MpdataError) as e:
            fn(*a, **kw)
        return e.value.code

    p = new_plan(M, name)
    assert code(p.column_scan, 0, 1) == M.ESTATE                                 # never filled
    upload(p, inp)
    L = M.lib()
    err = L.mpdata_last_error

    def state():
        import torch
        sh = M.shapes(*shape, ntr)
        t = {k: torch.empty(sh[k], dtype=H.tdt(dt), device="cuda:0") for k in ("f", "flux")}
        p.export_device(**t)
        p.sync()
        return {k: to_host(v) for k, v in t.items()}

    before = state()
    # (u, w, rho, rhow, adz have no export: the run behind the refused calls shows them, compared with the model's)
    bad = []
    raw = lambda sl0=0, n=ncrms, src=0, dst=1, mode=0: L.mpdata_plan_column_scan_device(p._p, sl0, n, src, dst, None, None, mode)

    def refused(rc, want, word=None):
        assert rc == want, (rc, want, err())
        text = err()
        assert word is None or word in text, (word, text)
        now = state()
        for k in before:
            assert_bitwise(now[k], before[k], f"after a refused call ({text!r}): {k}")
        bad.append(text)

    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, ncrms + 1), (ncrms, 1), (3, 3)):
        refused(raw(sl0, n), M.EINVAL)
    for t in (-1, ntr):
        refused(raw(src=t), M.EINVAL, b"src")
        refused(raw(dst=t), M.EINVAL, b"dst")
    for mode in (4, 5, 8, -2):
        refused(raw(mode=mode), M.EINVAL, b"mode")
    # the order: the range, src, dst, the mode
    refused(raw(0, 0, 9, 9, 4), M.EINVAL, b"n = 0")
    refused(raw(src=9, dst=9, mode=4), M.EINVAL, b"src")
    refused(raw(dst=9, mode=4), M.EINVAL, b"dst")
    # a host form of the other precision; its arguments come first
    h32 = lambda src=0, dst=1, mode=0: L.mpdata_plan_column_scan_f32(p._p, 0, ncrms, src, dst, None, None, mode)
    refused(h32(), M.ESTATE)
    refused(h32(src=ntr), M.EINVAL, b"src")
    refused(h32(mode=4), M.EINVAL, b"mode")
    # the array forms: sizes, the block, f, wgt, then src, dst and the mode
    one = 8
    arr = lambda ncrms=4, nz=6, sl0=0, n=4, f=one, src=0, dst=1, wgt=one, mode=0: \
        L.mpdata_column_scan_device(ncrms, 5, nz, 3, sl0, n, f, src, dst, wgt, None, mode, None)
    refused(arr(nz=1, sl0=2, n=3, f=None, wgt=None, src=9), M.EINVAL, b"nz=1")
    refused(arr(sl0=2, n=3, f=None, wgt=None, src=9), M.EINVAL, b"outside")
    refused(arr(f=None, wgt=None, src=9), M.EINVAL, b"null f")
    refused(arr(wgt=None, src=9), M.EINVAL, b"null wgt")
    refused(arr(src=3, dst=3, mode=4), M.EINVAL, b"src")
    refused(arr(dst=3, mode=4), M.EINVAL, b"dst")
    refused(arr(mode=4), M.EINVAL, b"mode")
    assert len(set(bad)) >= 12
    # ... and the plan still works, its velocities and coefficients among it
    m = model_of(oracle, name)
    step(M, p, m, name, 31, 0, 1, False, DOWN, True, f"{name}: behind the refused calls")
    p.run()
    assert m.run() is None
    same_as_model(M, p, name, m, "behind the refused calls, scan, run")
    p.close()


# ---- 6. a multi-GPU handle is refused; the single-device plans of its shards take the call
def test_multi_gpu_handle_and_shard_plan(mpdata, oracle, monkeypatch):
    M = mpdata
    monkeypatch.delenv("MPDATA_MULTI_XFER", raising=False)
    name = "f64-nz72"
    shape, ntr, dt, _ = KINDS[name]
    ncrms, nx, nz = shape
    inp = inputs(oracle, name)
    p = M.Plan(*shape, ntr, dtype=dt, devices=[0, 0])
    upload(p, inp)
    m = model_of(oracle, name)
    w = CS.make_wgt(ncrms, nz, dt, 540)
    with pytest.raises(M.MpdataError) as e:
        p.column_scan(0, 1, to_dev(w))
    assert e.value.code == M.EUNSUPPORTED and b"mpdata_plan_shard_plan" in M.lib().mpdata_last_error()
    with pytest.raises(M.MpdataError) as e:
        p.column_scan_host(0, 1, w)
    assert e.value.code == M.EUNSUPPORTED
    with pytest.raises(M.MpdataError) as e:
        p.column_scan(9, 9, mode=4)                              # (the handle comes before src, dst and the mode)
    assert e.value.code == M.EUNSUPPORTED
    same_as_model(M, p, name, m, "after the refused handle calls")
    for g, (_, s0, nloc) in enumerate(p.shards()):
        q = p.shard_plan(g)
        src, dst, given, mode, _ = BCALLS[g]
        wg = wgt_of(name, 41 + g, given, s0, nloc)
        want = model_scan(m, src, dst, wg, mode, s0, nloc)
        got = scan(M, q, name, src, dst, wg, mode, 0, nloc, call=q.column_scan)
        assert_bitwise(got, want, f"shard {g}: total")
        q.close()
    same_as_model(M, p, name, m, "after the shard plans' calls")
    p.run()
    assert m.run() is None
    same_as_model(M, p, name, m, "after the shard plans' calls and a run")
    p.close()


# ---- 7. the Fortran program: every record of its dump against the model
# dtype, program, shape, block, (src, dst)
FORTRAN = {
    "f64": (F64, "column_scan_calls", (7, 5, 10), (2, 3), (0, 2)), "f32": (F32, "column_scan_calls_sp", (6, 5, 10), (1, 3), (2, 0)),
    "f32-odd-ref": (F32, "column_scan_calls_sp", (7, 3, 12), (6, 1), (0, 2)), "f64-nz72": (F64, "column_scan_calls", (3, 2, 72), (1, 2), (2, 0)),
}


@pytest.mark.parametrize("case", list(FORTRAN))
def test_fortran_program_matches_the_model(oracle, tmp_path, case):
    """the program's calls: t1 into dst on the block, upward, with wgt and total; dst in place on the whole plan, downward
    and exclusive, without wgt; the host form: dst into t1 on the block, downward; a call with an unknown mode bit, refused"""
    dt, exe, shape, (sl0, n), (t1, dst) = FORTRAN[case]
    ncrms, nx, nz = shape
    inp = CS.make_plan_inputs(oracle, shape, T, dt, SEED + 3)
    wgt_a, wgt_c = CS.make_wgt(n, nz, dt, 700), CS.make_wgt(n, nz, dt, 701)
    records = [("params", np.array([ncrms, nx, nz, T, sl0, n, t1, dst], np.int64))]
    records += [(k, inp[k]) for k in PM.NAMES] + [("wgt_a", wgt_a), ("wgt_c", wgt_c)]
    # the replay on the model
    m = CS.PlanModelColumnScan(oracle, ncrms, nx, nz, T, dt)
    want = FR.want_import(m, inp)
    rc = lambda what, code=None: want.append(FR.rc(what, code))
    total_a = model_scan(m, t1, dst, wgt_a, UP, sl0, n)
    rc("scan_block"); rc("sync")
    want += [("total_a", total_a)]
    total_b = model_scan(m, dst, dst, None, DOWN | EXCL)
    rc("scan_dn_excl"); rc("sync")
    want += [("total_b", total_b)]
    total_c = model_scan(m, dst, t1, wgt_c, DOWN, sl0, n)
    rc("scan_host")
    want += [("total_c", total_c)]
    rc("scan_badmode", m.column_scan(t1, dst, None, 4))
    want += FR.want_close(m)
    FR.compare_dump(FR.run_program(exe, records, tmp_path), want, case)
