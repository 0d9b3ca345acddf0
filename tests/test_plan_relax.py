"""GPU tests of the relaxation of a resident plan's tracers to a level profile (include/mpdata_hip.h 3r):
mpdata_plan_relax_device, the host forms, the array forms, their Python face Plan.relax / relax_host / relax, and the
Fortran program tests/fortran/relax_calls.F90.

Every comparison is bit for bit (util.assert_bitwise) against the numpy model of tests/relax_model.py: RM.relax on a
reference-layout truth, or the plan model with the new call (RM.PlanModelRelax: an EXACT plan's f and flux are
bit-identical to it), or, for FAST plans, the plan's own whole export before the call.  c and target lie inside larger
buffers with 4 KiB of NaN on both sides, so a read outside the block's arrays poisons the result; mean is filled with NaN
and lies between two patterned bands of 4 KiB, which must come back unchanged, and so must c and target.  c is zero on the
lower half of the levels and in (0, 1] above, another value per instance and level; target is uniform in [-0.5, 0.5); f is
the oracle's raw field moved by one half, so signed.  Before every call the test asserts ON THE MODEL that the call
changes 10 % .. 90 % of the touched cells.  u and w have no export: that they keep their bits shows in the run behind every
call, which is compared with the model's.

A test first replays its script on the model -- that pass asserts the changed share and records what the plan must return
-- and then on the plan.

Shapes (ncrms, nx, nz), the smallest at which a path of the kernel differs (NB = 8 columns in flight):
  (5, 3, 8)        padding slots of an 8-instance tile, one short batch
  (5, 11, 28)      two column batches, the last short
  (3, 8, 28)       exactly one batch
  (3, 17, 28)      three batches, the last of one column
  (3, 3, 64), (3, 2, 65), (3, 9, 72), (2, 2, 140), (2, 2, 238)   63 elements; element 63 | 64 across two slices; three
                   and four slices with idle lanes and an idle wave
  (37, 3, 28)      19 tiles: more than one thread block of four waves, the last partly filled
  fp32             pairs (even), the phantom (odd with the switch), the reference layout (odd without it)
  windowed plans   (nz > 238 with set_tall_columns): 239 and 300 levels, 18 instances, fp32 with 15 pseudo-instances (an
                   inner phantom); 250 levels without the switch is a reference-layout plan.
Mean mode has two forms: up to nx = 32 the columns of an element stay in registers between the sum and the update (loads
in groups of 8: the shapes above are one short group, one whole group, two and three groups), above it f is read twice.
  (3, 32, 28), (6, 32, 28) fp32    the bound: four whole groups
  (3, 33, 28)      one above: the re-read form, five batches, the last of one column
  (3, 40, 28), (5, 43, 8)          the re-read form with five whole batches; six, the last short, with padding slots
  (7, 33, 28) fp32 odd, (2, 33, 239) tall   the re-read form with pairs, the phantom, split pairs and level windows"""
import numpy as np
import pytest

import fortran_records as FR
import plan_harness as H
import relax_model as RM
from oracle import plan_model as PM
from plan_harness import BAND, _defaults, nan_banded, nan_out, upload
from util import assert_bitwise, to_dev, to_host

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32

# name -> (shape, tracers, dtype, switches)
KINDS = {
    "f64-nz8": ((5, 3, 8), 2, F64, {}), "f64-nz28-nx11": ((5, 11, 28), 2, F64, {}), "f64-nz28-nx8": ((3, 8, 28), 1, F64, {}),
    "f64-nz28-nx17": ((3, 17, 28), 1, F64, {}), "f64-nz64": ((3, 3, 64), 1, F64, {}),
    "f64-nz65": ((3, 2, 65), 1, F64, {}), "f64-nz72": ((3, 9, 72), 2, F64, {}), "f64-nz140": ((2, 2, 140), 1, F64, {}),
    "f64-nz238": ((2, 2, 238), 1, F64, {}), "f64-nz28-5blocks": ((37, 3, 28), 1, F64, {}),
    "f64-nz28-nx32": ((3, 32, 28), 1, F64, {}), "f64-nz28-nx33": ((3, 33, 28), 2, F64, {}), "f64-nz28-nx40": ((3, 40, 28), 1, F64, {}),
    "f64-nz8-nx43": ((5, 43, 8), 1, F64, {}), "f32-nz28-nx32-even": ((6, 32, 28), 1, F32, {}),
    "f32-nz28-nx33-odd": ((7, 33, 28), 2, F32, dict(odd=True)), "f64-nz239-nx33-tall": ((2, 33, 239), 1, F64, dict(tall=True)),
    "f32-nz28-even": ((6, 3, 28), 2, F32, {}), "f32-nz28-5blocks": ((74, 3, 28), 1, F32, {}),
    "f32-nz72-even": ((4, 2, 72), 1, F32, {}),
    "f32-nz28-odd": ((7, 3, 28), 2, F32, dict(odd=True)), "f32-nz72-odd": ((3, 2, 72), 1, F32, dict(odd=True)),
    "f64-nz12-ref": ((5, 3, 12), 2, F64, dict(ref=True)), "f32-nz12-ref": ((6, 3, 12), 2, F32, dict(ref=True)),
    "f32-nz12-odd-ref": ((7, 3, 12), 1, F32, {}),      # (an odd fp32 plan without the switch keeps the reference layout)
    "f64-nz250-ref": ((2, 3, 250), 1, F64, {}),        # (above 238 levels without the switch: the reference layout)
    "f64-nz239-tall": ((2, 3, 239), 2, F64, dict(tall=True)), "f64-nz300-tall": ((3, 2, 300), 1, F64, dict(tall=True)),
    "f64-nz239-tall-18": ((18, 2, 239), 1, F64, dict(tall=True)),
    "f32-nz239-tall-odd": ((3, 2, 239), 2, F32, dict(tall=True, odd=True)),
}
REF = ("f32-nz12-odd-ref", "f64-nz12-ref", "f32-nz12-ref", "f64-nz250-ref")
# one kind of each family (and of the re-read form) runs the FAST variant too; five kinds run a PERIODIC plan
FAST = ("f64-nz28-nx11", "f64-nz72", "f32-nz28-odd", "f64-nz12-ref", "f64-nz239-tall", "f64-nz28-nx33")
PERIODIC = ("f64-nz28-nx11", "f32-nz72-odd", "f64-nz12-ref", "f32-nz239-tall-odd", "f32-nz28-nx33-odd")
SEED = 100


_INPUTS = {}


def inputs(oracle, name):
    """the seven arrays of KINDS[name]: computed once and shared; no test writes them"""
    if name not in _INPUTS:
        shape, T, dt, _ = KINDS[name]
        _INPUTS[name] = RM.make_plan_inputs(oracle, shape, T, dt, SEED)
    return _INPUTS[name]


def new_plan(M, name, variant=None):
    return H.new_plan(M, KINDS[name], name, name in REF, bool(KINDS[name][3].get("tall")), variant)


def model_of(oracle, name, inp=None):
    shape, T, dt, _ = KINDS[name]
    m = RM.PlanModelRelax(oracle, *shape, T, dt)
    assert m.upload({k: np.array(v, order="F") for k, v in (inp or inputs(oracle, name)).items()}) is None
    return m


def whole(M, p, name, what=("f", "flux")):
    return H.whole(M, p, KINDS[name], what)


def c_of(name, k, n=None):
    """c (n, nzm) of a block, other values per k"""
    shape, T, dt, _ = KINDS[name]
    return RM.make_c(shape[0] if n is None else n, shape[2], dt, 500 + k)


def t_of(name, k, n=None, ntr=None):
    """target (n, nzm, ntr) of a block, another profile per k"""
    shape, T, dt, _ = KINDS[name]
    return RM.make_target(shape[0] if n is None else n, shape[2], T if ntr is None else ntr, dt, 500 + k)


def relax(M, p, name, c, target=None, sl0=0, n=None, first=0, ntr=None, mean=True, lead=None, call=None):
    """Plan.relax of host c (n, nzm) and target (n, nzm, ntr) or None -> mean (n, nzm, ntr) or None; c, target and the
    bands are checked.  call: another callable with Plan.relax's arguments (a shard plan's)."""
    import torch
    shape, T, dt, _ = KINDS[name]
    nx, nz = shape[1], shape[2]
    n = shape[0] - sl0 if n is None else n
    ntr = T - first if ntr is None else ntr
    assert c.shape == (n, nz - 1) and c.dtype == dt
    assert target is None or (target.shape == (n, nz - 1, ntr) and target.dtype == dt)
    lead = (ntr != 1) if lead is None else lead
    sh = M.relax_shapes(n, nx, nz, ntr if lead else None)
    craw, cview = nan_banded(c, sh["c"])
    traw, tview = nan_banded(target, sh["target"]) if target is not None else (None, None)
    corig, torig = craw.clone(), None if traw is None else traw.clone()
    buf = nan_out(sh["mean"], dt) if mean else None
    torch.cuda.synchronize()      # (the plan may run on a stream that does not wait for the one that filled the buffers)
    (call or p.relax)(cview, tview, buf[2] if buf else None, sl0, n, first, ntr)
    p.sync()
    torch.cuda.synchronize()
    assert torch.equal(craw.view(torch.uint8), corig.view(torch.uint8)), "c changed"
    assert traw is None or torch.equal(traw.view(torch.uint8), torig.view(torch.uint8)), "target changed"
    if not buf:
        return None
    raw, pristine, view = buf
    assert torch.equal(raw[:BAND], pristine[:BAND]) and torch.equal(raw[-BAND:], pristine[-BAND:]), "mean: a band byte changed"
    return to_host(view).reshape((n, nz - 1, ntr), order="F")


def model_relax(m, name, c, target=None, sl0=0, n=None, first=0, ntr=None):
    """the call on the plan model -> mean; that it changes 10 % .. 90 % of the touched cells is asserted first"""
    frac = RM.changed_fraction(m.a["f"], c, target, sl0, n, first, ntr)
    assert 0.1 <= frac <= 0.9, (name, sl0, n, first, ntr, frac)
    mean = m.relax(c, target, sl0=sl0, n=n, first=first, ntr=ntr)
    assert not isinstance(mean, int), mean
    return mean


def snap(m):
    return {k: np.array(v, order="F") for k, v in m.export_device().items()}


def same(got, want, what):
    for k in ("f", "flux"):
        assert_bitwise(got[k], want[k], f"{what}: {k}")


# ---- 1. every kind of plan: whole plan, both modes, with and without mean, every state, a run behind every call
# the script: (target, mean, k of the inputs); the first behind the upload, the others behind a run (a windowed plan's seams are stale)
SCRIPT = ((False, True, 0), (True, True, 1), (False, False, 2), (True, False, 3))
PSCRIPT = ((5, True), (6, False), (7, True), (8, False))   # (k, target) on the PERIODIC plan


@pytest.mark.parametrize("name", list(KINDS))
def test_every_plan_kind(mpdata, oracle, name):
    M = mpdata
    shape, T, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    inp = inputs(oracle, name)
    F0 = inp["f"].reshape((ncrms, nx + 6, nz - 1, T), order="F")
    assert (F0 < 0).any() and (F0 > 0).any()
    # ---- the model's pass
    m = model_of(oracle, name)
    want = []
    for tgt, mean, k in SCRIPT:
        c, t = c_of(name, k), t_of(name, k) if tgt else None
        assert (c == 0).any() and (c > 0).any()
        before = np.array(m.a["f"], order="F")
        mn = model_relax(m, name, c, t)
        new_f, new_m = RM.relax(before, c, t)
        assert_bitwise(m.a["f"], new_f, "the plan model is the operator")
        assert_bitwise(mn, new_m, "the plan model's mean")
        assert_bitwise(new_f[:, :3], before[:, :3], "the halos stay")
        assert_bitwise(new_f[:, nx + 3:], before[:, nx + 3:], "the halos stay")
        after_call = snap(m)
        assert m.run() is None
        want.append((mn, after_call, snap(m)))
    per = []
    if name in PERIODIC:
        assert m.set_boundary(PM.PERIODIC) is None
        assert m.run() is None
        for k, tgt in PSCRIPT:
            mn = model_relax(m, name, c_of(name, k), t_of(name, k) if tgt else None)
            if k == 7:
                assert m.run() is None
            if k == 8:
                assert m.set_boundary(PM.GIVEN) is None
            per.append((mn, snap(m)))
    # ---- the plan's pass
    p = new_plan(M, name)
    upload(p, inp)
    for (tgt, mean, k), (wm, w_call, w_run) in zip(SCRIPT, want):
        got = relax(M, p, name, c_of(name, k), t_of(name, k) if tgt else None, mean=mean)
        if mean:
            assert_bitwise(got, wm, f"{name} script {k}: mean")
        same(whole(M, p, name), w_call, f"{name} script {k} (target {tgt}, mean {mean}): the call")
        # a run on the kept velocities = export -> model -> import -> run: seams and the phantom are consistent
        p.run()
        same(whole(M, p, name), w_run, f"{name} script {k} (target {tgt}, mean {mean}): the call, run")
    if name in PERIODIC:
        p.set_boundary(M.BOUNDARY_PERIODIC)
        p.run()
        # (5) the halos are stale behind the run; the export hands out wrapped halos of the NEW field
        # (6) on halos the export just wrapped: they are copies of the OLD field now, the next export wraps again
        # (7) a run right behind the call, no read-back between   (8) back to GIVEN behind a call: the plan holds what an
        # export just before the switch would have returned
        for (k, tgt), (wm, w) in zip(PSCRIPT, per):
            got = relax(M, p, name, c_of(name, k), t_of(name, k) if tgt else None, mean=k != 7)
            if got is not None:
                assert_bitwise(got, wm, f"{name} periodic {k}: mean")
            if k == 7:
                p.run()
            if k == 8:
                p.set_boundary(M.BOUNDARY_GIVEN)
            e = whole(M, p, name)
            same(e, w, f"{name} periodic {k}")
            if k in (5, 6):
                assert_bitwise(e["f"], PM.wrap(np.array(e["f"], order="F")), f"{name} periodic {k}: the halos are wrapped copies of the new interior")
    p.close()
    if name in FAST:
        # FAST: the same bits as EXACT on the uploaded f; after a run against the plan's own export changed by the model
        p = new_plan(M, name, variant=M.VARIANT_FAST)
        upload(p, inp)
        assert_bitwise(relax(M, p, name, c_of(name, 0)), want[0][0], f"{name} FAST: mean")
        assert_bitwise(whole(M, p, name, ("f",))["f"], want[0][1]["f"], f"{name} FAST upload, relax")
        p.run()
        for k, tgt in ((1, True), (2, False)):
            E = whole(M, p, name, ("f",))["f"]
            c, t = c_of(name, k), t_of(name, k) if tgt else None
            assert 0.1 <= RM.changed_fraction(E, c, t) <= 0.9
            got = relax(M, p, name, c, t)
            want_E, m_E = RM.relax(E, c, t)
            assert_bitwise(got, m_E, f"{name} FAST run, relax {k}: mean")
            assert_bitwise(whole(M, p, name, ("f",))["f"], want_E, f"{name} FAST run, relax {k}")
        p.close()


# ---- 2. blocks and tracer sub-ranges: what lies outside keeps every bit
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
    # fp32 pairs, odd plan of 7 (instance 6 shares its pair with the phantom): blocks that hold and miss instance 6
    "f32-nz28-odd": [(1, 2), (6, 1), (5, 2), (0, 6), (3, 3), (0, 7)],
    "f32-nz72-odd": [(2, 1), (1, 1), (0, 2)],
    # the re-read form of mean mode (nx = 33): padding slots, split pairs and the phantom, level windows
    "f64-nz8-nx43": [(1, 3), (4, 1)],
    "f32-nz28-nx33-odd": [(1, 2), (6, 1), (5, 2), (0, 7)],
    "f64-nz239-nx33-tall": [(1, 1), (0, 1), (0, 2)],
    "f32-nz12-odd-ref": [(1, 3), (6, 1)],
    "f64-nz12-ref": [(1, 3), (4, 1)],
    # windowed plans: each behind an import (the first) and behind a run (the others: stale seams), a block and the whole
    "f64-nz239-tall": [(1, 1), (0, 1), (0, 2)],
    "f64-nz239-tall-18": [(15, 3), (17, 1), (1, 16)],
    "f32-nz239-tall-odd": [(1, 1), (2, 1), (0, 2), (0, 3)],
}
# the first block of these splits an fp32 pair at one end at least: the instances next to it, the partner among them,
# hold -0.0 and negative values
SPLIT = {"f32-nz28-even": (0, 4), "f32-nz28-5blocks": (14, 34), "f32-nz28-odd": (0, 3), "f32-nz28-nx33-odd": (0, 3)}
# the windowed fp32 kind takes its -0.0 by a block import behind the last run and is read back without another run, as in
# test_plan_cell_add.py (a run of a windowed fp32 plan may turn a -0.0 into +0.0; nothing of this call is involved)
SPLIT_TALL = {"f32-nz239-tall-odd": ((0, 2), (1, 1))}


@pytest.mark.parametrize("name", list(BLOCKS))
def test_blocks_leave_the_rest_alone(mpdata, oracle, name):
    """the modes alternate from mean mode; mean on two calls of three.  Kinds of SPLIT: the uploaded f of the partner
    instances holds -0.0 on every second level of column 1 and negative values elsewhere."""
    M = mpdata
    shape, T, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    inp = dict(inputs(oracle, name))
    if name in SPLIT:
        f = np.array(inp["f"], order="F")
        for b in SPLIT[name]:
            f[b, 3, ::2] = -0.0
            assert (f[b, 3:nx + 3] < 0).any()
        inp["f"] = f
    calls = []
    for k, (sl0, n) in enumerate(BLOCKS[name]):
        first, ntr = ((k % T), 1) if T > 1 else (0, 1)
        if T > 1 and k == len(BLOCKS[name]) - 1:
            first, ntr = 0, T
        calls.append((k, sl0, n, first, ntr, k % 2 == 1, k % 3 != 2))
    # ---- the model's pass
    m = model_of(oracle, name, inp)
    want = []
    for k, sl0, n, first, ntr, tgt, mean in calls:
        before = snap(m)
        c, t = c_of(name, 10 + k, n), t_of(name, 10 + k, n, ntr) if tgt else None
        mn = model_relax(m, name, c, t, sl0, n, first, ntr)
        after = snap(m)
        new = RM.relax(before["f"][sl0:sl0 + n, ..., first:first + ntr], c, t)[0]
        assert_bitwise(after["f"][sl0:sl0 + n, ..., first:first + ntr], new, "inside")
        assert m.run() is None
        want.append((mn, before, after, snap(m)))
    # ---- the plan's pass
    p = new_plan(M, name)
    upload(p, inp)
    for (k, sl0, n, first, ntr, tgt, mean), (wm, w_before, w_after, w_run) in zip(calls, want):
        what = f"{name} block {sl0, n} tracers {first, ntr} target {tgt}"
        before = whole(M, p, name)
        same(before, w_before, what + ": before")
        got = relax(M, p, name, c_of(name, 10 + k, n), t_of(name, 10 + k, n, ntr) if tgt else None, sl0, n, first, ntr, mean=mean,
                    lead=bool(k % 2) or ntr > 1)
        if mean:
            assert_bitwise(got, wm, what + ": mean")
        after = whole(M, p, name)
        out = np.ones(ncrms, bool)
        out[sl0:sl0 + n] = False
        tout = np.ones(T, bool)
        tout[first:first + ntr] = False
        assert_bitwise(after["f"][out], before["f"][out], what + ": instances outside")
        assert_bitwise(after["f"][..., tout], before["f"][..., tout], what + ": tracers outside")
        assert_bitwise(after["flux"], before["flux"], what + ": flux")
        same(after, w_after, what + ": the call")
        if k == 0 and name in SPLIT:
            for b in SPLIT[name]:
                assert out[b] and np.all(np.signbit(after["f"][b, 3, ::2, first]) & (after["f"][b, 3, ::2, first] == 0)), b
                assert (after["f"][b, 3:nx + 3, :, first] < 0).any(), b
        # a run of every instance (the phantom of an odd plan rides with instance ncrms - 1; a windowed plan refreshes
        # the seams the call marked stale; u, w, rho, rhow, adz enter it) matches the model
        p.run()
        same(whole(M, p, name), w_run, what + ": the call, run")
    if name in SPLIT_TALL:
        # stale seams behind the run; the neighbours take -0.0 by a block import, the block between them is relaxed
        outside, (sl0, n) = SPLIT_TALL[name]
        for b in outside:
            fb = np.array(m.export_block(b, 1, ("f",), 0, T)["f"], order="F")
            fb[0, 3, ::2], fb[0, 4, ::2] = -0.0, -0.25
            p.import_block(b, f=to_dev(fb if T > 1 else fb[..., 0]))
            assert m.import_block(b, 1, {"f": fb}, 0, T) is None
        c = c_of(name, 19, n)
        wm = model_relax(m, name, c, None, sl0, n)
        assert_bitwise(relax(M, p, name, c, None, sl0, n), wm, f"{name}: mean beside -0.0")
        e = whole(M, p, name)
        same(e, snap(m), f"{name}: the call beside -0.0")
        for b in outside:
            assert np.all(np.signbit(e["f"][b, 3, ::2]) & (e["f"][b, 3, ::2] == 0)) and np.all(e["f"][b, 4, ::2] == -0.25), b
    p.close()


# ---- 2b. a level with c == 0 is not rewritten: its -0.0 stay.  Computed through, such a level gives x - 0 * (x - m), and
# for x = -0.0 below a positive m that is -0.0 - (-0.0) = +0.0: the only bits by which a kernel that drops the guard differs.
@pytest.mark.parametrize("name", ["f64-nz28-nx11", "f64-nz28-nx33", "f32-nz28-odd", "f32-nz28-nx33-odd", "f64-nz12-ref", "f64-nz239-tall"])
def test_c_zero_levels_keep_negative_zero(mpdata, oracle, name):
    M = mpdata
    shape, T, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    half = (nz - 1) // 2
    inp = dict(inputs(oracle, name))
    f = np.array(inp["f"], order="F")
    f[:, 3:nx + 3, :half] = np.abs(f[:, 3:nx + 3, :half]) + dt(0.5)      # the levels with c == 0: positive, so m > 0 ...
    f[:, 3, :half] = -0.0                                                # ... but for columns 1 and 3
    f[:, 5, :half] = -0.0
    inp["f"] = f
    m = model_of(oracle, name, inp)
    p = new_plan(M, name)
    upload(p, inp)
    for k, tgt in ((0, False), (1, True)):
        c = c_of(name, 50 + k)
        assert not c[:, :half].any() and c[:, half:].all()
        t = np.asfortranarray(np.abs(t_of(name, 50 + k)) + dt(0.25)) if tgt else None
        wm = m.relax(c, t)
        assert not isinstance(wm, int) and (wm[:, :half] > 0).all()
        got = relax(M, p, name, c, t)
        assert_bitwise(got, wm, f"{name} target {tgt}: mean")
        e = whole(M, p, name)
        same(e, snap(m), f"{name} target {tgt}: the call")
        for col in (3, 5):
            assert np.all(np.signbit(e["f"][:, col, :half]) & (e["f"][:, col, :half] == 0)), (name, tgt, col)
    p.close()


# ---- 3. the host form and the array forms
@pytest.mark.parametrize("name", ["f64-nz28-nx11", "f32-nz28-odd", "f64-nz12-ref", "f64-nz72", "f64-nz239-tall", "f64-nz28-nx33"])
def test_host_form(mpdata, oracle, name):
    M = mpdata
    shape, T, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    tail = (T,) if T > 1 else ()
    script = ((0, ncrms, False, True), (1, 1, True, False), (ncrms - 1, 1, False, True), (0, 2, True, True))
    m = model_of(oracle, name)
    want = []
    for k, (sl0, n, tgt, mean) in enumerate(script):
        mn = model_relax(m, name, c_of(name, 20 + k, n), t_of(name, 20 + k, n) if tgt else None, sl0, n)
        after = snap(m)
        assert m.run() is None
        want.append((mn, after, snap(m)))
    p = new_plan(M, name)
    upload(p, inputs(oracle, name))
    for k, ((sl0, n, tgt, mean), (wm, w_call, w_run)) in enumerate(zip(script, want)):
        c = c_of(name, 20 + k, n)
        th = np.asfortranarray(t_of(name, 20 + k, n).reshape((n, nz - 1) + tail, order="F")) if tgt else None
        keep_c, keep_t = np.array(c, order="F"), None if th is None else np.array(th, order="F")
        mh = np.full((n, nz - 1) + tail, np.nan, dt, order="F") if mean else None
        p.relax_host(c, th, mh, sl0, n)
        assert_bitwise(c, keep_c, f"{name} host {sl0, n}: c")
        if th is not None:
            assert_bitwise(th, keep_t, f"{name} host {sl0, n}: target")
        if mh is not None:
            assert_bitwise(mh.reshape(wm.shape, order="F"), wm, f"{name} host {sl0, n}: mean")
        same(whole(M, p, name), w_call, f"{name} host form {sl0, n}")
        p.run()
        same(whole(M, p, name), w_run, f"{name} host form {sl0, n}, run")
    with pytest.raises(M.MpdataError):
        p.relax_host(c[:, :-1], sl0=0, n=2)              # a wrong shape
    p.close()


# 257 and 600 instances: more than one block of 256 threads and a partly filled last one; (2, 1, 3) with 32769 tracers:
# 65538 rows, the second trip over gridDim.y.  f, c and target are random, so instance b differs from b - 256 and row r
# from r - 65535.  Each with a block inside the arrays.
ARRAYS = {"n257": ((257, 3, 6), 2, (1, 256)), "n600": ((600, 2, 5), 1, (300, 299)), "rows65538": ((2, 1, 3), 32769, (1, 1))}


@pytest.mark.parametrize("case", list(ARRAYS))
@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
def test_array_forms(mpdata, dt, case):
    import torch
    M = mpdata
    (ncrms, nx, nz), T, (b0, bn) = ARRAYS[case]
    rng = np.random.default_rng([77, ncrms, T])
    f = np.asfortranarray(rng.uniform(-0.5, 0.5, (ncrms, nx + 6, nz - 1, T)).astype(dt))
    for (sl0, n), tgt in (((0, ncrms), False), ((b0, bn), True)):
        c = RM.make_c(n, nz, dt, 600 + sl0)
        if nz - 1 < 4:
            c[:, 0] = 0                                      # (two levels: one of them stays)
        t = RM.make_target(n, nz, T, dt, 600 + sl0) if tgt else None
        if nx > 1 or tgt:
            assert 0.1 <= RM.changed_fraction(f[sl0:sl0 + n], c, t) <= 0.9
        want, want_m = RM.relax(f[sl0:sl0 + n], c, t)
        full = np.array(f, order="F")
        full[sl0:sl0 + n] = want
        if n > 256:
            assert not np.array_equal(want[256:], want[:n - 256]) and not np.array_equal(want_m[256:], want_m[:n - 256])
        if T > 32768:
            assert not np.array_equal(want_m[..., 32768:], want_m[..., :T - 32768])
        fd = to_dev(f)
        sh = M.relax_shapes(n, nx, nz, T)
        craw, cview = nan_banded(c, sh["c"])
        traw, tview = nan_banded(t, sh["target"]) if tgt else (None, None)
        corig, torig = craw.clone(), None if traw is None else traw.clone()
        bd = nan_out(sh["mean"], dt)
        torch.cuda.synchronize()
        M.relax(fd, cview, tview, bd[2], sl0, n)
        torch.cuda.synchronize()
        assert torch.equal(bd[0][:BAND], bd[1][:BAND]) and torch.equal(bd[0][-BAND:], bd[1][-BAND:])
        assert torch.equal(craw.view(torch.uint8), corig.view(torch.uint8)), "c changed"
        assert traw is None or torch.equal(traw.view(torch.uint8), torig.view(torch.uint8)), "target changed"
        assert_bitwise(to_host(fd), full, f"array form {case} block {sl0, n}: f")
        assert_bitwise(to_host(bd[2]), want_m, f"array form {case} block {sl0, n}: mean")
    if T == 1 or case == "n257":
        # one tracer without the tracer axis, mean skipped
        f1 = to_dev(np.asfortranarray(f[..., 0]))
        c = RM.make_c(ncrms, nz, dt, 650)
        M.relax(f1, to_dev(c))
        torch.cuda.synchronize()
        assert_bitwise(to_host(f1), RM.relax(f[..., 0], c)[0], f"array form {case}, one tracer: f")


# ---- 4. every error code, in the stated order; the plan's state before and after
def test_errors_change_nothing(mpdata, oracle):
    M = mpdata
    name = "f64-nz28-nx11"
    shape, T, dt, _ = KINDS[name]
    ncrms, nx, nz = shape
    inp = inputs(oracle, name)
    w = to_dev(c_of(name, 30))

    def code(fn, *a, **kw):
        with pytest.raises(M.MpdataError) as e:
            fn(*a, **kw)
        return e.value.code

    p = new_plan(M, name)
    assert code(p.relax, w) == M.ESTATE                                          # never filled
    upload(p, inp)
    before = whole(M, p, name)
    L = M.lib()
    raw = lambda sl0, n, first, ntr, c=w.data_ptr(): L.mpdata_plan_relax_device(p._p, sl0, n, c, None, None, first, ntr)
    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, ncrms + 1), (ncrms, 1), (3, 3)):
        assert raw(sl0, n, 0, 1) == M.EINVAL, (sl0, n)
    for first, ntr in ((0, 0), (-1, 1), (1, 2), (2, 1), (0, 3)):
        assert raw(0, ncrms, first, ntr) == M.EINVAL, (first, ntr)
    assert raw(0, ncrms, 0, 1, None) == M.EINVAL and b"null c" in L.mpdata_last_error()
    assert raw(0, 0, 0, 1, None) == M.EINVAL and b"n = 0" in L.mpdata_last_error()                # the range first
    assert raw(0, ncrms, 0, 3, None) == M.EINVAL and b"tracer range" in L.mpdata_last_error()     # then the tracers
    # a host form of the other precision; its NULL comes first
    c32 = np.asfortranarray(c_of(name, 30).astype(F32))
    assert L.mpdata_plan_relax_f32(p._p, 0, ncrms, c32.ctypes.data, None, None) == M.ESTATE
    assert L.mpdata_plan_relax_f32(p._p, 0, ncrms, None, None, None) == M.EINVAL and b"null c" in L.mpdata_last_error()
    # the array forms: sizes, the block, f, then c
    one = 8
    arr = L.mpdata_relax_device
    assert arr(4, 5, 1, 1, 0, 4, None, None, None, None, None) == M.EINVAL and b"nz=1" in L.mpdata_last_error()
    assert arr(4, 5, 6, 1, 2, 3, None, None, None, None, None) == M.EINVAL and b"outside" in L.mpdata_last_error()
    assert arr(4, 5, 6, 1, 0, 4, None, None, None, None, None) == M.EINVAL and b"null f" in L.mpdata_last_error()
    assert arr(4, 5, 6, 1, 0, 4, one, None, None, None, None) == M.EINVAL and b"null c" in L.mpdata_last_error()
    after = whole(M, p, name)
    for k in before:
        assert_bitwise(after[k], before[k], f"after the refused calls: {k}")
    p.relax(w)                                                                   # ... and the plan still works
    p.sync()
    assert not np.array_equal(whole(M, p, name, ("f",))["f"], before["f"])
    p.close()


# ---- 5. a multi-GPU handle is refused; the single-device plans of its shards take the call
def test_multi_gpu_handle_and_shard_plan(mpdata, oracle, monkeypatch):
    M = mpdata
    monkeypatch.delenv("MPDATA_MULTI_XFER", raising=False)
    name = "f64-nz28-nx11"
    shape, T, dt, _ = KINDS[name]
    ncrms, nx, nz = shape
    inp = inputs(oracle, name)
    p = M.Plan(*shape, T, dtype=dt, devices=[0, 0])
    upload(p, inp)
    m = model_of(oracle, name)
    w = c_of(name, 40)
    with pytest.raises(M.MpdataError) as e:
        p.relax(to_dev(w))
    assert e.value.code == M.EUNSUPPORTED and b"mpdata_plan_shard_plan" in M.lib().mpdata_last_error()
    with pytest.raises(M.MpdataError) as e:
        p.relax_host(w)
    assert e.value.code == M.EUNSUPPORTED
    same(whole(M, p, name), m.export_device(), "after the refused handle calls")
    for g, (_, s0, nloc) in enumerate(p.shards()):
        q = p.shard_plan(g)
        cg, tg = c_of(name, 41 + g, nloc), t_of(name, 41 + g, nloc) if g else None
        want = model_relax(m, name, cg, tg, s0, nloc)
        got = relax(M, q, name, cg, tg, 0, nloc, call=q.relax)
        assert_bitwise(got, want, f"shard {g}: mean")
        q.close()
    same(whole(M, p, name), m.export_device(), "after the shard plans' calls")
    p.run()
    assert m.run() is None
    same(whole(M, p, name), m.export_device(), "after the shard plans' calls and a run")
    p.close()


# ---- 6. the Fortran program: every record of its dump against the model
FORTRAN = {
    "f64": (F64, "relax_calls", (7, 5, 10), 3, (2, 3), (1, 2)), "f32": (F32, "relax_calls_sp", (6, 5, 10), 3, (1, 3), (1, 2)),
    "f64-whole": (F64, "relax_calls", (5, 3, 28), 2, (0, 5), (0, 2)), "f32-odd-ref": (F32, "relax_calls_sp", (7, 3, 12), 2, (6, 1), (1, 1)),
    "f64-nz72": (F64, "relax_calls", (3, 2, 72), 1, (1, 2), (0, 1)), "f32-nz72": (F32, "relax_calls_sp", (4, 2, 72), 2, (1, 2), (0, 2)),
}


@pytest.mark.parametrize("case", list(FORTRAN))
def test_fortran_program_matches_the_model(oracle, tmp_path, case):
    """the program's calls: to the horizontal mean on the block, all tracers; to a target on the whole plan, a tracer range"""
    dt, exe, shape, T, (sl0, n), (t1, tn) = FORTRAN[case]
    ncrms, nx, nz = shape
    inp = RM.make_plan_inputs(oracle, shape, T, dt, SEED + 3)
    arrs = {k: (inp[k].reshape(inp[k].shape + (1,), order="F") if T == 1 and k in ("f", "flux") else inp[k]) for k in PM.NAMES}
    c_a = RM.make_c(n, nz, dt, 700)
    c_b = RM.make_c(ncrms, nz, dt, 701)
    tgt_b = RM.make_target(ncrms, nz, tn, dt, 702)
    records = [("params", np.array([ncrms, nx, nz, T, sl0, n, t1, tn], np.int64))]
    records += [(k, arrs[k]) for k in PM.NAMES] + [("c_a", c_a), ("c_b", c_b), ("tgt_b", tgt_b)]
    # the replay on the model
    m = RM.PlanModelRelax(oracle, ncrms, nx, nz, T, dt)
    want = FR.want_import(m, inp)
    rc = lambda what, code=None: want.append(FR.rc(what, code))
    mean_a = model_relax(m, case, c_a, None, sl0, n)
    rc("relax_block"); rc("sync")
    want += [("mean_a", mean_a)]
    mean_b = model_relax(m, case, c_b, tgt_b, 0, ncrms, t1, tn)
    assert_bitwise(mean_b, tgt_b, "mean is the target")
    rc("relax_range"); rc("sync")
    want += [("mean_b", mean_b)]
    want += FR.want_close(m)
    FR.compare_dump(FR.run_program(exe, records, tmp_path), want, case)
