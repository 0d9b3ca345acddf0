"""GPU tests of the first-order conversion between two tracers of a resident plan (include/mpdata_hip.h 3t):
mpdata_plan_convert_device, the host forms, the array forms, their Python face Plan.convert / convert_host / convert, and
the Fortran program tests/fortran/convert_calls.F90.

Every comparison is bit for bit (util.assert_bitwise) against the numpy model of tests/convert_model.py: CV.convert on a
reference-layout truth, or the plan model with the new call (CV.PlanModelConvert: an EXACT plan's f and flux are
bit-identical to it), or, for FAST plans, the plan's own whole export before the call.  r, q0 and y lie inside larger
buffers with 4 KiB of NaN on both sides, so a read outside the block's arrays poisons the result; dsum is filled with NaN
and lies between two patterned bands of 4 KiB, which must come back unchanged, and so must r, q0 and y.  r is zero on the
lower half of the levels and in (0, 2] above, another value per instance and level; q0 is the lower median of the src
row, so some cells have a == q0 exactly; y is uniform in [0.5, 1.5); f is the oracle's raw field moved by one half, so
signed, with -0.0 planted in every tracer (the array forms take the raw field).  Before every call the test asserts ON THE
MODEL that the call changes 10 % .. 90 % of the touched cells of src, that the e <= 0 branch is taken in at least 10 % of
the cells of the converting levels and, in LIMIT calls, that the cap is active in at least 10 % of the converted cells.  u
and w have no export: that they keep their bits shows in the run behind every call, which is compared with the model's.

Plans have three tracers; the pairs are (0, 2), (2, 0) and (1, 0) -- non-adjacent, reversed (the negative stride between
the two streams) and adjacent --, and the third tracer must keep every bit.

A test first replays its script on the model -- that pass asserts the shares and records what the plan must return -- and
then on the plan.

Shapes (ncrms, nx, nz), the smallest at which a path of the kernel differs (NB = 8 columns in flight on each stream):
  (5, 3, 8)        padding slots of an 8-instance tile, one short batch
  (3, 8, 28)       exactly one batch
  (5, 11, 28)      two column batches, the last short
  (3, 17, 28)      three batches, the last of one column
  (3, 3, 64), (3, 2, 65), (3, 9, 72), (2, 2, 140), (2, 2, 238)   63 elements; element 63 | 64 across two slices; three
                   and four slices with idle lanes and an idle wave
  (37, 3, 28), fp32 (74, 3, 28)   19 tiles: more than one thread block of four waves, the last partly filled
  fp32             pairs (even), the phantom (odd with the switch), the reference layout (odd without it)
  windowed plans   (nz > 238 with set_tall_columns): 239 and 300 levels, 18 instances, fp32 with 15 pseudo-instances (an
                   inner phantom); 250 levels without the switch is a reference-layout plan."""
import numpy as np
import pytest

import convert_model as CV
import fortran_records as FR
import plan_harness as H
from oracle import plan_model as PM
from plan_harness import BAND, _defaults, nan_banded, nan_out, upload
from util import assert_bitwise, to_dev, to_host

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
T = 3

# name -> (shape, tracers, dtype, switches)
KINDS = {
    "f64-nz8": ((5, 3, 8), T, F64, {}), "f64-nz28-nx8": ((3, 8, 28), T, F64, {}), "f64-nz28-nx11": ((5, 11, 28), T, F64, {}),
    "f64-nz28-nx17": ((3, 17, 28), T, F64, {}), "f64-nz64": ((3, 3, 64), T, F64, {}), "f64-nz65": ((3, 2, 65), T, F64, {}),
    "f64-nz72": ((3, 9, 72), T, F64, {}), "f64-nz140": ((2, 2, 140), T, F64, {}), "f64-nz238": ((2, 2, 238), T, F64, {}),
    "f64-nz28-5blocks": ((37, 3, 28), T, F64, {}), "f32-nz28-5blocks": ((74, 3, 28), T, F32, {}),
    "f32-nz28-even": ((6, 3, 28), T, F32, {}), "f32-nz72-even": ((4, 2, 72), T, F32, {}),
    "f32-nz28-odd": ((7, 3, 28), T, F32, dict(odd=True)), "f32-nz72-odd": ((3, 2, 72), T, F32, dict(odd=True)),
    "f64-nz12-ref": ((5, 3, 12), T, F64, dict(ref=True)), "f32-nz12-ref": ((6, 3, 12), T, F32, dict(ref=True)),
    "f32-nz12-odd-ref": ((7, 3, 12), T, F32, {}),      # (an odd fp32 plan without the switch keeps the reference layout)
    "f64-nz250-ref": ((2, 3, 250), T, F64, {}),        # (above 238 levels without the switch: the reference layout)
    "f64-nz239-tall": ((2, 3, 239), T, F64, dict(tall=True)), "f64-nz300-tall": ((3, 2, 300), T, F64, dict(tall=True)),
    "f64-nz239-tall-18": ((18, 2, 239), T, F64, dict(tall=True)),
    "f32-nz239-tall-odd": ((3, 2, 239), T, F32, dict(tall=True, odd=True)),
}
REF = ("f32-nz12-odd-ref", "f64-nz12-ref", "f32-nz12-ref", "f64-nz250-ref")
# one kind of each family runs the FAST variant too; five kinds run a PERIODIC plan
FAST = ("f64-nz28-nx11", "f64-nz72", "f32-nz28-odd", "f64-nz12-ref", "f64-nz239-tall")
PERIODIC = ("f64-nz28-nx11", "f32-nz72-odd", "f64-nz12-ref", "f32-nz239-tall-odd", "f64-nz28-nx17")
PAIRS = ((0, 2), (2, 0), (1, 0))
SEED = 100


_INPUTS = {}


def inputs(oracle, name):
    """the seven arrays of KINDS[name]: computed once and shared; no test writes them"""
    if name not in _INPUTS:
        shape, ntr, dt, _ = KINDS[name]
        _INPUTS[name] = CV.make_plan_inputs(oracle, shape, ntr, dt, SEED)
    return _INPUTS[name]


def new_plan(M, name, variant=None):
    return H.new_plan(M, KINDS[name], name, name in REF, bool(KINDS[name][3].get("tall")), variant)


def model_of(oracle, name, inp=None):
    shape, ntr, dt, _ = KINDS[name]
    m = CV.PlanModelConvert(oracle, *shape, ntr, dt)
    assert m.upload({k: np.array(v, order="F") for k, v in (inp or inputs(oracle, name)).items()}) is None
    return m


def whole(M, p, name, what=("f", "flux")):
    return H.whole(M, p, KINDS[name], what)


def args_of(name, k, F, src, q0, y, sl0=0, n=None):
    """(r, q0, y) of a call on block [sl0, sl0 + n) of the field F (ncrms, nx+6, nzm, T), other values per k; q0 is made
    from the field the call meets"""
    shape, _, dt, _ = KINDS[name]
    n = shape[0] - sl0 if n is None else n
    return (CV.make_r(n, shape[2], dt, 500 + k), CV.make_q0(F[sl0:sl0 + n, ..., src]) if q0 else None,
            CV.make_y(n, shape[2], dt, 500 + k) if y else None)


def convert(M, p, name, src, dst, r, q0=None, y=None, mode=0, sl0=0, n=None, dsum=True, call=None):
    """Plan.convert of host r, q0, y (n, nzm) -> dsum (n, nzm) or None; r, q0, y and the bands are checked.  call: another
    callable with Plan.convert's arguments (a shard plan's)."""
    import torch
    shape, _, dt, _ = KINDS[name]
    nx, nz = shape[1], shape[2]
    n = shape[0] - sl0 if n is None else n
    for a in (r, q0, y):
        assert a is None or (a.shape == (n, nz - 1) and a.dtype == dt)
    sh = M.convert_shapes(n, nx, nz)
    ins = {k: nan_banded(a, sh[k]) for k, a in (("r", r), ("q0", q0), ("y", y)) if a is not None}
    orig = {k: raw.clone() for k, (raw, _) in ins.items()}
    buf = nan_out(sh["dsum"], dt) if dsum else None
    view = lambda k: ins[k][1] if k in ins else None
    torch.cuda.synchronize()      # (the plan may run on a stream that does not wait for the one that filled the buffers)
    (call or p.convert)(src, dst, view("r"), view("q0"), view("y"), mode, buf[2] if buf else None, sl0, n)
    p.sync()
    torch.cuda.synchronize()
    for k, (raw, _) in ins.items():
        assert torch.equal(raw.view(torch.uint8), orig[k].view(torch.uint8)), f"{k} changed"
    if not buf:
        return None
    raw, pristine, out = buf
    assert torch.equal(raw[:BAND], pristine[:BAND]) and torch.equal(raw[-BAND:], pristine[-BAND:]), "dsum: a band byte changed"
    return to_host(out).reshape((n, nz - 1), order="F")


def assert_shares(F, name, src, dst, r, q0, y, mode, sl0=0, n=None):
    """the three preconditions of a call, on the field it meets"""
    changed, off, cap = CV.branch_shares(F, src, dst, r, q0, y, bool(mode & CV.LIMIT), sl0, n)
    assert 0.1 <= changed <= 0.9, (name, src, dst, mode, sl0, n, "changed", changed)
    assert off >= 0.1, (name, src, dst, mode, sl0, n, "e <= 0", off)
    assert not (mode & CV.LIMIT) or cap >= 0.1, (name, src, dst, mode, sl0, n, "cap", cap)


def model_convert(m, name, src, dst, r, q0=None, y=None, mode=0, sl0=0, n=None):
    """the call on the plan model -> dsum; the three shares are asserted first"""
    assert_shares(m.a["f"], name, src, dst, r, q0, y, mode, sl0, n)
    dsum = m.convert(src, dst, r, q0, y, mode, sl0=sl0, n=n)
    assert not isinstance(dsum, int), dsum
    return dsum


def model_run(m):
    """a run of the model.  The plan kernels and the oracle do not agree on the sign of the zero a run returns for a cell that
    held -0.0 and met no flux (the run's clamp at zero; nothing of this call is involved), so the -0.0 of the inputs are
    planted where no run of these scripts returns a -0.0: asserted here, on the model"""
    assert m.run() is None
    f = m.a["f"]
    assert not np.signbit(f[f == 0]).any(), "a run returns -0.0: plant the -0.0 of the inputs elsewhere"


def snap(m):
    return {k: np.array(v, order="F") for k, v in m.export_device().items()}


def same(got, want, what):
    for k in ("f", "flux"):
        assert_bitwise(got[k], want[k], f"{what}: {k}")


# ---- 1. every kind of plan: whole plan, the four forms of the call, every state, a run behind every call
# the script: (pair, q0, y, mode, dsum, k of the inputs): all optional arguments; none; LIMIT; LIMIT without q0.  The first
# behind the upload, the others behind a run (a windowed plan's seams are stale)
SCRIPT = (((0, 2), True, True, 0, True, 0), ((2, 0), False, False, 0, False, 1), ((1, 0), True, True, CV.LIMIT, True, 2),
          ((0, 2), False, True, CV.LIMIT, True, 3))
PSCRIPT = ((5, (0, 2), True, 0), (6, (2, 0), False, 0), (7, (1, 0), True, CV.LIMIT), (8, (0, 2), False, CV.LIMIT))   # (k, pair, q0 and y, mode)


@pytest.mark.parametrize("name", list(KINDS))
def test_every_plan_kind(mpdata, oracle, name):
    M = mpdata
    shape, ntr, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    inp = inputs(oracle, name)
    F0 = inp["f"]
    assert F0.shape == (ncrms, nx + 6, nz - 1, T) and (F0 < 0).any() and (F0 > 0).any() and np.signbit(F0[F0 == 0]).any()
    # ---- the model's pass
    m = model_of(oracle, name)
    want = []
    for (src, dst), q0, y, mode, ds, k in SCRIPT:
        a = args_of(name, k, m.a["f"], src, q0, y)
        assert (a[0] == 0).any() and (a[0] > 1).any()
        before = np.array(m.a["f"], order="F")
        dsum = model_convert(m, name, src, dst, *a, mode)
        new_f, new_s = CV.convert(before, src, dst, *a, bool(mode))
        assert_bitwise(m.a["f"], new_f, "the plan model is the operator")
        assert_bitwise(dsum, new_s, "the plan model's dsum")
        assert_bitwise(new_f[:, :3], before[:, :3], "the halos stay")
        assert_bitwise(new_f[:, nx + 3:], before[:, nx + 3:], "the halos stay")
        assert_bitwise(new_f[..., 3 - src - dst], before[..., 3 - src - dst], "the third tracer stays")
        after_call = snap(m)
        model_run(m)
        want.append((a, dsum, after_call, snap(m)))
    per = []
    if name in PERIODIC:
        assert m.set_boundary(PM.PERIODIC) is None
        model_run(m)
        for k, (src, dst), opt, mode in PSCRIPT:
            a = args_of(name, k, m.a["f"], src, opt, opt)
            dsum = model_convert(m, name, src, dst, *a, mode)
            if k == 7:
                model_run(m)
            if k == 8:
                assert m.set_boundary(PM.GIVEN) is None
            per.append((a, dsum, snap(m)))
    # ---- the plan's pass
    p = new_plan(M, name)
    upload(p, inp)
    for ((src, dst), q0, y, mode, ds, k), (a, wsum, w_call, w_run) in zip(SCRIPT, want):
        what = f"{name} script {k} (pair {src, dst}, q0 {q0}, y {y}, mode {mode})"
        before = whole(M, p, name, ("f",))["f"]
        got = convert(M, p, name, src, dst, *a, mode, dsum=ds)
        if ds:
            assert_bitwise(got, wsum, what + ": dsum")
        e = whole(M, p, name)
        assert_bitwise(e["f"][..., 3 - src - dst], before[..., 3 - src - dst], what + ": the third tracer")
        same(e, w_call, what + ": the call")
        # a run on the kept velocities = export -> model -> import -> run: seams and the phantom are consistent
        p.run()
        same(whole(M, p, name), w_run, what + ": the call, run")
    if name in PERIODIC:
        p.set_boundary(M.BOUNDARY_PERIODIC)
        p.run()
        # (5) the halos are stale behind the run; the export hands out wrapped halos of the NEW fields
        # (6) on halos the export just wrapped: they are copies of the OLD fields now, the next export wraps again
        # (7) a run right behind the call, no read-back between   (8) back to GIVEN behind a call: the plan holds what an
        # export just before the switch would have returned
        for (k, (src, dst), opt, mode), (a, wsum, w) in zip(PSCRIPT, per):
            got = convert(M, p, name, src, dst, *a, mode, dsum=k != 7)
            if got is not None:
                assert_bitwise(got, wsum, f"{name} periodic {k}: dsum")
            if k == 7:
                p.run()
            if k == 8:
                p.set_boundary(M.BOUNDARY_GIVEN)
            e = whole(M, p, name)
            same(e, w, f"{name} periodic {k}")
            if k in (5, 6):
                assert_bitwise(e["f"], PM.wrap(np.array(e["f"], order="F")),
                               f"{name} periodic {k}: the halos are wrapped copies of the new interior, in both tracers")
    p.close()
    if name in FAST:
        # FAST: the same bits as EXACT on the uploaded f; after a run against the plan's own export changed by the model
        p = new_plan(M, name, variant=M.VARIANT_FAST)
        upload(p, inp)
        (src, dst), _, _, mode, _, _ = SCRIPT[0]
        assert_bitwise(convert(M, p, name, src, dst, *want[0][0], mode), want[0][1], f"{name} FAST: dsum")
        assert_bitwise(whole(M, p, name, ("f",))["f"], want[0][2]["f"], f"{name} FAST upload, convert")
        p.run()
        for k, (src, dst), opt, mode in ((1, (2, 0), False, 0), (2, (1, 0), True, CV.LIMIT)):
            E = whole(M, p, name, ("f",))["f"]
            a = args_of(name, k, E, src, opt, opt)
            assert_shares(E, name, src, dst, *a, mode)
            got = convert(M, p, name, src, dst, *a, mode)
            want_E, s_E = CV.convert(E, src, dst, *a, bool(mode))
            assert_bitwise(got, s_E, f"{name} FAST run, convert {k}: dsum")
            assert_bitwise(whole(M, p, name, ("f",))["f"], want_E, f"{name} FAST run, convert {k}")
        p.close()


# ---- 2. blocks: what lies outside keeps every bit
BLOCKS = {
    # eight instances per tile, five instances: inside the tile, one instance, the last one
    "f64-nz8": [(1, 3), (2, 1), (4, 1), (0, 5)],
    # two per tile: mid-tile to mid-tile, the last (half-filled) tile
    "f64-nz28-nx11": [(1, 3), (4, 1), (0, 4)],
    # 19 tiles in five thread blocks: a block of instances across thread blocks, odd ends, the last instance alone
    "f64-nz28-5blocks": [(7, 11), (3, 32), (36, 1), (8, 8)],
    "f64-nz72": [(1, 1), (1, 2)],
    "f64-nz140": [(1, 1), (0, 1)],
    # fp32 pairs: a block that splits pairs at both ends
    "f32-nz28-even": [(1, 3), (5, 1), (2, 2)],
    "f32-nz28-5blocks": [(15, 19), (1, 72), (73, 1)],
    # fp32 pairs, odd plan of 7 (instance 6 shares its pair with the phantom): blocks that hold and miss instance 6, the
    # single-instance block of instance 6 among them
    "f32-nz28-odd": [(1, 2), (6, 1), (5, 2), (0, 6), (3, 3), (0, 7)],
    "f32-nz72-odd": [(2, 1), (1, 1), (0, 2)],
    "f32-nz12-odd-ref": [(1, 3), (6, 1)],
    "f64-nz12-ref": [(1, 3), (4, 1)],
    # windowed plans: each behind an import (the first) and behind a run (the others: stale seams), a block and the whole
    "f64-nz239-tall": [(1, 1), (0, 1), (0, 2)],
    "f64-nz239-tall-18": [(15, 3), (17, 1), (1, 16)],
    "f32-nz239-tall-odd": [(1, 1), (2, 1), (0, 2), (0, 3)],
}
# the first block of these splits an fp32 pair at one end at least: the instances next to it, the partner among them,
# hold -0.0 and negative values in every tracer
SPLIT = {"f32-nz28-even": (0, 4), "f32-nz28-5blocks": (14, 34), "f32-nz28-odd": (0, 3)}


@pytest.mark.parametrize("name", list(BLOCKS))
def test_blocks_leave_the_rest_alone(mpdata, oracle, name):
    """the pairs and the forms of the call rotate; dsum on two calls of three.  Kinds of SPLIT: the uploaded f of the partner
    instances holds -0.0 on every second level of column 1 (CV.plant_negative_zeros) and negative values elsewhere."""
    M = mpdata
    shape, ntr, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    inp = dict(inputs(oracle, name))
    planted = np.zeros(inp["f"].shape, bool)
    if name in SPLIT:
        for b in SPLIT[name]:
            planted[b, 3, ::2] = True
            assert (inp["f"][b, 3:nx + 3] < 0).any()
        inp, planted = CV.plant_negative_zeros(oracle, inp, planted | (inp["f"] == 0))
        planted[:, 4] = False                                # (the -0.0 every input has: not looked at below)
        assert all(planted[b].sum() >= T * ((nz - 1) // 4) for b in SPLIT[name])
    calls = []
    for k, (sl0, n) in enumerate(BLOCKS[name]):
        opt = k % 2 == 0
        # (a block of one instance has too few converted cells for the cap's share to be asserted: it takes the plain mode)
        calls.append((k, sl0, n, PAIRS[k % 3], opt, opt or k % 4 == 1, CV.LIMIT if n > 1 and k % 4 in (1, 2) else 0, k % 3 != 2))
    # ---- the model's pass
    m = model_of(oracle, name, inp)
    want = []
    for k, sl0, n, (src, dst), q0, y, mode, ds in calls:
        before = snap(m)
        a = args_of(name, 10 + k, m.a["f"], src, q0, y, sl0, n)
        dsum = model_convert(m, name, src, dst, *a, mode, sl0, n)
        after = snap(m)
        new = CV.convert(before["f"][sl0:sl0 + n], src, dst, *a, bool(mode))[0]
        assert_bitwise(after["f"][sl0:sl0 + n], new, "inside")
        model_run(m)
        want.append((a, dsum, before, after, snap(m)))
    # ---- the plan's pass
    p = new_plan(M, name)
    upload(p, inp)
    for (k, sl0, n, (src, dst), q0, y, mode, ds), (a, wsum, w_before, w_after, w_run) in zip(calls, want):
        what = f"{name} block {sl0, n} pair {src, dst} mode {mode}"
        before = whole(M, p, name)
        same(before, w_before, what + ": before")
        got = convert(M, p, name, src, dst, *a, mode, sl0, n, dsum=ds)
        if ds:
            assert_bitwise(got, wsum, what + ": dsum")
        after = whole(M, p, name)
        out = np.ones(ncrms, bool)
        out[sl0:sl0 + n] = False
        assert_bitwise(after["f"][out], before["f"][out], what + ": instances outside")
        assert_bitwise(after["f"][..., 3 - src - dst], before["f"][..., 3 - src - dst], what + ": the third tracer")
        assert_bitwise(after["flux"], before["flux"], what + ": flux")
        same(after, w_after, what + ": the call")
        if k == 0 and name in SPLIT:
            for b in SPLIT[name]:
                assert out[b] and np.all(np.signbit(after["f"][b][planted[b]]) & (after["f"][b][planted[b]] == 0)), b
                assert all((after["f"][b, 3:nx + 3, :, t] < 0).any() for t in range(T)), b
        # a run of every instance (the phantom of an odd plan rides with instance ncrms - 1; a windowed plan refreshes
        # the seams the call marked stale; u, w, rho, rhow, adz enter it) matches the model
        p.run()
        same(whole(M, p, name), w_run, what + ": the call, run")
    p.close()


# ---- 2b. a level with r == 0 is not rewritten: its -0.0 stay in both tracers.  Computed through, such a level gives
# c + 0 * e = c + 0, and for c = -0.0 that is +0.0 (and a - +0 keeps a): the only bits by which a kernel that drops the guard
# differs are the -0.0 of dst.
@pytest.mark.parametrize("name", ["f64-nz28-nx11", "f32-nz28-odd", "f64-nz12-ref", "f64-nz239-tall"])
def test_r_zero_levels_keep_negative_zero(mpdata, oracle, name):
    M = mpdata
    shape, ntr, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    half = (nz - 1) // 2
    inp = dict(inputs(oracle, name))
    f = np.array(inp["f"], order="F")
    f[:, 3, :half] = -0.0                                                # the levels with r == 0: columns 1 and 3, every tracer
    f[:, 5, :half] = -0.0
    inp["f"] = f
    m = model_of(oracle, name, inp)
    p = new_plan(M, name)
    upload(p, inp)
    for k, (src, dst), opt, mode in ((0, (0, 2), True, 0), (1, (2, 0), False, CV.LIMIT)):
        a = args_of(name, 50 + k, m.a["f"], src, opt, opt)
        assert not a[0][:, :half].any() and a[0][:, half:].all()
        wsum = m.convert(src, dst, *a, mode)
        assert not isinstance(wsum, int) and not wsum[:, :half].any() and not np.signbit(wsum[:, :half]).any()
        got = convert(M, p, name, src, dst, *a, mode)
        assert_bitwise(got, wsum, f"{name} pair {src, dst}: dsum")
        e = whole(M, p, name)
        same(e, snap(m), f"{name} pair {src, dst}: the call")
        for col in (3, 5):
            assert np.all(np.signbit(e["f"][:, col, :half]) & (e["f"][:, col, :half] == 0)), (name, src, dst, col)
    p.close()


# ---- 3. the host form and the array forms
@pytest.mark.parametrize("name", ["f64-nz28-nx11", "f32-nz28-odd", "f64-nz12-ref", "f64-nz72", "f64-nz239-tall"])
def test_host_form(mpdata, oracle, name):
    M = mpdata
    shape, ntr, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    # (sl0, n, pair, q0 and y, mode, dsum)
    script = ((0, ncrms, (0, 2), True, 0, True), (1, ncrms - 1, (2, 0), False, CV.LIMIT, False), (ncrms - 1, 1, (1, 0), True, 0, True),
              (0, 2, (0, 2), True, CV.LIMIT, True))
    m = model_of(oracle, name)
    want = []
    for k, (sl0, n, (src, dst), opt, mode, ds) in enumerate(script):
        a = args_of(name, 20 + k, m.a["f"], src, opt, opt, sl0, n)
        dsum = model_convert(m, name, src, dst, *a, mode, sl0, n)
        after = snap(m)
        model_run(m)
        want.append((a, dsum, after, snap(m)))
    p = new_plan(M, name)
    upload(p, inputs(oracle, name))
    for (sl0, n, (src, dst), opt, mode, ds), (a, wsum, w_call, w_run) in zip(script, want):
        keep = [None if x is None else np.array(x, order="F") for x in a]
        sh = np.full((n, nz - 1), np.nan, dt, order="F") if ds else None
        p.convert_host(src, dst, *a, mode, sh, sl0, n)
        for x, kx, nm in zip(a, keep, ("r", "q0", "y")):
            if x is not None:
                assert_bitwise(x, kx, f"{name} host {sl0, n}: {nm}")
        if sh is not None:
            assert_bitwise(sh, wsum, f"{name} host {sl0, n}: dsum")
        same(whole(M, p, name), w_call, f"{name} host form {sl0, n}")
        p.run()
        same(whole(M, p, name), w_run, f"{name} host form {sl0, n}, run")
    with pytest.raises(M.MpdataError):
        p.convert_host(0, 2, a[0][:, :-1], sl0=0, n=2)       # a wrong shape
    p.close()


# 257 and 600 instances: more than one block of 256 threads and a partly filled last one; (2, 1, 70000): the second trip over
# gridDim.y.  f and the coefficients are random, so instance b differs from b - 256 and level k from k - 65535.  Each with a
# block inside the arrays (sl0 > 0).  f is the raw field, in [0, 1), with -0.0 planted.
ARRAYS = {"n257": ((257, 3, 6), 3, (1, 256)), "n600": ((600, 2, 5), 4, (300, 299)), "rows70000": ((2, 1, 70000), 3, (1, 1))}


@pytest.mark.parametrize("case", list(ARRAYS))
@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
def test_array_forms(mpdata, dt, case):
    import torch
    M = mpdata
    (ncrms, nx, nz), ntr, (b0, bn) = ARRAYS[case]
    rng = np.random.default_rng([77, ncrms, ntr])
    f = rng.uniform(0.0, 1.0, (ncrms, nx + 6, nz - 1, ntr)).astype(dt)
    f[:, 3, ::3] = -0.0
    f = np.asfortranarray(f)
    for (sl0, n), (src, dst), mode in (((0, ncrms), (0, ntr - 1), 0), ((b0, bn), (ntr - 1, 1), CV.LIMIT)):
        r, y = CV.make_r(n, nz, dt, 600 + sl0), CV.make_y(n, nz, dt, 600 + sl0)
        # the threshold with the plain call (nx = 1: the lower median is the cell itself and nothing would convert; half of
        # it); the LIMIT call without one: on a field in [0, 1) the cap bites where r > 1, and the cells that take the e <= 0
        # branch are the planted zeros
        q0 = None if mode else CV.make_q0(f[sl0:sl0 + n, ..., src]) if nx > 1 else np.asfortranarray(f[sl0:sl0 + n, 3, :, src] * dt(0.5))
        if nx > 1 or mode:
            assert_shares(f, case, src, dst, r, q0, y, mode, sl0, n)
        want, want_s = CV.convert(f[sl0:sl0 + n], src, dst, r, q0, y, bool(mode))
        full = np.array(f, order="F")
        full[sl0:sl0 + n] = want
        assert not np.array_equal(full, f)
        if n > 256:
            assert not np.array_equal(want[256:], want[:n - 256]) and not np.array_equal(want_s[256:], want_s[:n - 256])
        if nz - 1 > 65535:
            assert not np.array_equal(want_s[:, 65535:], want_s[:, :nz - 1 - 65535])
        fd = to_dev(f)
        sh = M.convert_shapes(n, nx, nz)
        ins = {k: nan_banded(a, sh[k]) for k, a in (("r", r), ("q0", q0), ("y", y)) if a is not None}
        orig = {k: raw.clone() for k, (raw, _) in ins.items()}
        bd = nan_out(sh["dsum"], dt)
        torch.cuda.synchronize()
        M.convert(fd, src, dst, ins["r"][1], ins["q0"][1] if q0 is not None else None, ins["y"][1], mode, bd[2], sl0, n)
        torch.cuda.synchronize()
        assert torch.equal(bd[0][:BAND], bd[1][:BAND]) and torch.equal(bd[0][-BAND:], bd[1][-BAND:])
        for k, (raw, _) in ins.items():
            assert torch.equal(raw.view(torch.uint8), orig[k].view(torch.uint8)), f"{k} changed"
        assert_bitwise(to_host(fd), full, f"array form {case} block {sl0, n}: f")
        assert_bitwise(to_host(bd[2]), want_s, f"array form {case} block {sl0, n}: dsum")
        f = full
    # r alone, dsum skipped
    fd = to_dev(f)
    r = CV.make_r(ncrms, nz, dt, 650)
    M.convert(fd, 1, 0, to_dev(r))
    torch.cuda.synchronize()
    assert_bitwise(to_host(fd), CV.convert(f, 1, 0, r)[0], f"array form {case}, r alone: f")


# ---- 4. every error code, in the stated order; the plan's state before and after
def test_errors_change_nothing(mpdata, oracle):
    M = mpdata
    name = "f64-nz28-nx11"
    shape, ntr, dt, _ = KINDS[name]
    ncrms, nx, nz = shape
    inp = inputs(oracle, name)
    w = to_dev(CV.make_r(ncrms, nz, dt, 530))

    def code(fn, *a, **kw):
        with pytest.raises(M.MpdataError) as e:
            fn(*a, **kw)
        return e.value.code

    p = new_plan(M, name)
    assert code(p.convert, 0, 2, w) == M.ESTATE                                  # never filled
    upload(p, inp)
    before = whole(M, p, name)
    L = M.lib()
    err = L.mpdata_last_error
    raw = lambda sl0=0, n=ncrms, src=0, dst=2, r=w.data_ptr(), mode=0: L.mpdata_plan_convert_device(p._p, sl0, n, src, dst, r, None, None, mode, None)
    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, ncrms + 1), (ncrms, 1), (3, 3)):
        assert raw(sl0, n) == M.EINVAL, (sl0, n)
    for src, dst in ((-1, 0), (0, -1), (3, 0), (0, 3)):
        assert raw(src=src, dst=dst) == M.EINVAL and b"tracer pair" in err(), (src, dst)
    for t in range(T):
        assert raw(src=t, dst=t) == M.EINVAL and b"src == dst" in err()
    assert raw(r=None) == M.EINVAL and b"null r" in err()
    for mode in (2, 3, 4, -2):
        assert raw(mode=mode) == M.EINVAL and b"mode" in err(), mode
    # the order: the range, the pair, src == dst, r, the mode
    assert raw(0, 0, 9, 9, None, 2) == M.EINVAL and b"n = 0" in err()
    assert raw(src=9, dst=9, r=None, mode=2) == M.EINVAL and b"tracer pair" in err()
    assert raw(src=1, dst=1, r=None, mode=2) == M.EINVAL and b"src == dst" in err()
    assert raw(r=None, mode=2) == M.EINVAL and b"null r" in err()
    # a host form of the other precision; its arguments come first
    r32 = np.asfortranarray(CV.make_r(ncrms, nz, F32, 530))
    h32 = lambda src=0, dst=2, r=r32.ctypes.data, mode=0: L.mpdata_plan_convert_f32(p._p, 0, ncrms, src, dst, r, None, None, mode, None)
    assert h32() == M.ESTATE
    assert h32(r=None) == M.EINVAL and b"null r" in err()
    assert h32(src=1, dst=1) == M.EINVAL and h32(mode=2) == M.EINVAL and h32(dst=3) == M.EINVAL
    # the array forms: sizes, the block, f, then the pair, r and the mode
    one = 8
    arr = lambda ncrms=4, nz=6, sl0=0, n=4, f=one, src=0, dst=2, r=one, mode=0: \
        L.mpdata_convert_device(ncrms, 5, nz, 3, sl0, n, f, src, dst, r, None, None, mode, None, None)
    assert arr(nz=1, sl0=2, n=3, f=None, r=None) == M.EINVAL and b"nz=1" in err()
    assert arr(sl0=2, n=3, f=None, r=None) == M.EINVAL and b"outside" in err()
    assert arr(f=None, src=1, dst=1, r=None) == M.EINVAL and b"null f" in err()
    assert arr(src=3, r=None) == M.EINVAL and b"tracer pair" in err()
    assert arr(src=1, dst=1, r=None) == M.EINVAL and b"src == dst" in err()
    assert arr(r=None, mode=2) == M.EINVAL and b"null r" in err()
    assert arr(mode=2) == M.EINVAL and b"mode" in err()
    after = whole(M, p, name)
    for k in before:
        assert_bitwise(after[k], before[k], f"after the refused calls: {k}")
    p.convert(0, 2, w)                                                           # ... and the plan still works
    p.sync()
    assert not np.array_equal(whole(M, p, name, ("f",))["f"], before["f"])
    p.close()


# ---- 5. a multi-GPU handle is refused; the single-device plans of its shards take the call
def test_multi_gpu_handle_and_shard_plan(mpdata, oracle, monkeypatch):
    M = mpdata
    monkeypatch.delenv("MPDATA_MULTI_XFER", raising=False)
    name = "f64-nz28-nx11"
    shape, ntr, dt, _ = KINDS[name]
    ncrms, nx, nz = shape
    inp = inputs(oracle, name)
    p = M.Plan(*shape, ntr, dtype=dt, devices=[0, 0])
    upload(p, inp)
    m = model_of(oracle, name)
    w = CV.make_r(ncrms, nz, dt, 540)
    with pytest.raises(M.MpdataError) as e:
        p.convert(0, 2, to_dev(w))
    assert e.value.code == M.EUNSUPPORTED and b"mpdata_plan_shard_plan" in M.lib().mpdata_last_error()
    with pytest.raises(M.MpdataError) as e:
        p.convert_host(0, 2, w)
    assert e.value.code == M.EUNSUPPORTED
    with pytest.raises(M.MpdataError) as e:
        p.convert(1, 1, to_dev(w))                           # (the handle comes before the pair)
    assert e.value.code == M.EUNSUPPORTED
    same(whole(M, p, name), m.export_device(), "after the refused handle calls")
    for g, (_, s0, nloc) in enumerate(p.shards()):
        q = p.shard_plan(g)
        src, dst = PAIRS[g + 1]
        a = args_of(name, 41 + g, m.a["f"], src, bool(g), bool(g), s0, nloc)
        want = model_convert(m, name, src, dst, *a, CV.LIMIT * g, s0, nloc)
        got = convert(M, q, name, src, dst, *a, CV.LIMIT * g, 0, nloc, call=q.convert)
        assert_bitwise(got, want, f"shard {g}: dsum")
        q.close()
    same(whole(M, p, name), m.export_device(), "after the shard plans' calls")
    p.run()
    model_run(m)
    same(whole(M, p, name), m.export_device(), "after the shard plans' calls and a run")
    p.close()


# ---- 6. the Fortran program: every record of its dump against the model
# dtype, program, shape, block, (src, dst)
FORTRAN = {
    "f64": (F64, "convert_calls", (7, 5, 10), (2, 3), (0, 2)), "f32": (F32, "convert_calls_sp", (6, 5, 10), (1, 3), (2, 0)),
    "f64-whole": (F64, "convert_calls", (5, 3, 28), (0, 5), (1, 0)), "f32-odd-ref": (F32, "convert_calls_sp", (7, 3, 12), (6, 1), (0, 2)),
    "f64-nz72": (F64, "convert_calls", (3, 2, 72), (1, 2), (2, 0)), "f32-nz72": (F32, "convert_calls_sp", (4, 2, 72), (1, 2), (0, 1)),
}


@pytest.mark.parametrize("case", list(FORTRAN))
def test_fortran_program_matches_the_model(oracle, tmp_path, case):
    """the program's calls: src -> dst on the block with q0, y and dsum; dst -> src on the whole plan, LIMIT, r alone, with
    dsum; a call with src == dst, refused"""
    dt, exe, shape, (sl0, n), (src, dst) = FORTRAN[case]
    ncrms, nx, nz = shape
    # (no -0.0 planted: behind the capped call a -0.0 next to cells that were emptied meets no flux in the program's run,
    # and the plan kernels and the oracle do not agree on the sign of the zero such a cell comes back with)
    inp = CV.make_plan_inputs(oracle, shape, T, dt, SEED + 3, zeros=False)
    r_a, y_a = CV.make_r(n, nz, dt, 700), CV.make_y(n, nz, dt, 700)
    q0_a = CV.make_q0(inp["f"][sl0:sl0 + n, ..., src])
    r_b = CV.make_r(ncrms, nz, dt, 701)
    records = [("params", np.array([ncrms, nx, nz, T, sl0, n, src, dst], np.int64))]
    records += [(k, inp[k]) for k in PM.NAMES] + [("r_a", r_a), ("q0_a", q0_a), ("y_a", y_a), ("r_b", r_b)]
    # the replay on the model
    m = CV.PlanModelConvert(oracle, ncrms, nx, nz, T, dt)
    want = FR.want_import(m, inp)
    rc = lambda what, code=None: want.append(FR.rc(what, code))
    dsum_a = model_convert(m, case, src, dst, r_a, q0_a, y_a, 0, sl0, n)
    rc("convert_block"); rc("sync")
    want += [("dsum_a", dsum_a)]
    dsum_b = model_convert(m, case, dst, src, r_b, None, None, CV.LIMIT)
    rc("convert_back"); rc("sync")
    want += [("dsum_b", dsum_b)]
    rc("convert_same", m.convert(src, src, r_b))
    want += FR.want_close(m)
    assert not np.signbit(m.a["f"][m.a["f"] == 0]).any(), "the run returns -0.0 (model_run)"
    FR.compare_dump(FR.run_program(exe, records, tmp_path), want, case)
