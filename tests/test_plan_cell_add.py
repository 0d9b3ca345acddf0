"""GPU tests of the per-cell sources of a resident plan (include/mpdata_hip.h 3p): mpdata_plan_cell_add_device, the host
forms, the array forms, their Python face Plan.cell_add / cell_add_host / cell_add, and the Fortran program
tests/fortran/cell_add_calls.F90.

Every comparison is bit for bit (util.assert_bitwise) against the numpy model of tests/cell_add_model.py: CM.cell_add on a
reference-layout truth, or the plan model with the new call (CM.PlanModelCellAdd: an EXACT plan's f and flux are
bit-identical to it), or, for FAST plans, the plan's own whole export before the call.  s lies inside a larger buffer with
4 KiB of NaN on both sides, so a read outside the block's array poisons the result; dsum is filled with NaN and lies
between two patterned bands of 4 KiB, which must come back unchanged, and so must s.  s is uniform in [-0.5, 0.5), another
value per cell and tracer; f is the oracle's raw field moved by one half, so signed; c = 0.75, and 0.1 -- no fp32 number,
the library rounds it once -- on the kind "f32-nz28-even".  Before every CLIP call the test asserts ON THE MODEL that the
clip acts on 10 % .. 90 % of the touched cells.  u and w have no export: that they keep their bits shows in the run behind
every call, which is compared with the model's.

A test first replays its script on the model -- that pass asserts the clip condition and records what the plan must
return -- and then on the plan.

G = 16 is the group of the kernel: the adjacent 8-byte elements of the instance axis a workgroup owns; it halves until two
LDS buffers of two columns fit beside the running sums of dsum, so a shape may run with another group with dsum than
without.  Shapes (ncrms, nx, nz), the smallest at which a path of the kernel differs:
  (5, 3, 8)        padding slots of an 8-instance tile, one batch
  (5, 11, 28)      batches of 5 columns: three of them, the last short, so the first LDS buffer is staged a second time
  (3, 3, 64)       63 elements, four rounds, batches of 2 and 1
  (2G+5, 3, 28)    three groups, the last short
  (3, 2, 65), (3, 9, 72)   element 63 | 64 across two waves; G = 8 with dsum (batches of 3), 16 without (batches of 2)
  (2, 2, 140)      three slices, an idle wave; G = 4 with dsum, 8 without
  (2, 2, 238)      four slices, G = 4
  fp32             pairs (even), 2G+3 pairs, the phantom (odd with the switch), the reference layout (odd without it)
  windowed plans   (nz > 238 with set_tall_columns): 239 and 300 levels, G+2 instances (two groups), fp32 with 15
                   pseudo-instances (an inner phantom); 250 levels without the switch is a reference-layout plan."""
import numpy as np
import pytest

import cell_add_model as CM
import fortran_records as FR
import plan_harness as H
from oracle import plan_model as PM
from plan_harness import BAND, _defaults, nan_banded, nan_out, upload
from util import assert_bitwise, to_dev, to_host

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
G = 16

# name -> (shape, tracers, dtype, switches)
KINDS = {
    "f64-nz8": ((5, 3, 8), 2, F64, {}), "f64-nz28-nx11": ((5, 11, 28), 2, F64, {}), "f64-nz64": ((3, 3, 64), 1, F64, {}),
    "f64-nz28-3groups": ((2 * G + 5, 3, 28), 1, F64, {}),
    "f64-nz65": ((3, 2, 65), 1, F64, {}), "f64-nz72": ((3, 9, 72), 2, F64, {}), "f64-nz140": ((2, 2, 140), 1, F64, {}),
    "f64-nz238": ((2, 2, 238), 1, F64, {}),
    "f32-nz28-even": ((6, 3, 28), 2, F32, {}), "f32-nz28-3groups": ((4 * G + 6, 3, 28), 1, F32, {}),
    "f32-nz72-even": ((4, 2, 72), 1, F32, {}),
    "f32-nz28-odd": ((7, 3, 28), 2, F32, dict(odd=True)), "f32-nz72-odd": ((3, 2, 72), 1, F32, dict(odd=True)),
    "f64-nz12-ref": ((5, 3, 12), 2, F64, dict(ref=True)), "f32-nz12-ref": ((6, 3, 12), 2, F32, dict(ref=True)),
    "f32-nz12-odd-ref": ((7, 3, 12), 1, F32, {}),      # (an odd fp32 plan without the switch keeps the reference layout)
    "f64-nz250-ref": ((2, 3, 250), 1, F64, {}),        # (above 238 levels without the switch: the reference layout)
    "f64-nz239-tall": ((2, 3, 239), 2, F64, dict(tall=True)), "f64-nz300-tall": ((3, 2, 300), 1, F64, dict(tall=True)),
    "f64-nz239-tall-2groups": ((G + 2, 2, 239), 1, F64, dict(tall=True)),
    "f32-nz239-tall-odd": ((3, 2, 239), 2, F32, dict(tall=True, odd=True)),
}
REF = ("f32-nz12-odd-ref", "f64-nz12-ref", "f32-nz12-ref", "f64-nz250-ref")
# one kind of each family runs the FAST variant too; four kinds run a PERIODIC plan
FAST = ("f64-nz28-nx11", "f64-nz72", "f32-nz28-odd", "f64-nz12-ref", "f64-nz239-tall")
PERIODIC = ("f64-nz28-nx11", "f32-nz72-odd", "f64-nz12-ref", "f32-nz239-tall-odd")
SEED = 100
ADD, CLIP = CM.ADD, CM.CLIP


def factor(name):
    """0.1 has no fp32 form: the kernel must round it once and multiply in fp32"""
    return 0.1 if name == "f32-nz28-even" else 0.75


_INPUTS = {}


def inputs(oracle, name):
    """the seven arrays of KINDS[name]: computed once and shared; no test writes them"""
    if name not in _INPUTS:
        shape, T, dt, _ = KINDS[name]
        _INPUTS[name] = CM.make_plan_inputs(oracle, shape, T, dt, SEED)
    return _INPUTS[name]


def new_plan(M, name, variant=None):
    return H.new_plan(M, KINDS[name], name, name in REF, bool(KINDS[name][3].get("tall")), variant)


def model_of(oracle, name, inp=None):
    shape, T, dt, _ = KINDS[name]
    m = CM.PlanModelCellAdd(oracle, *shape, T, dt)
    assert m.upload({k: np.array(v, order="F") for k, v in (inp or inputs(oracle, name)).items()}) is None
    return m


def whole(M, p, name, what=("f", "flux")):
    return H.whole(M, p, KINDS[name], what)


def s_of(name, k, n=None, ntr=None):
    """s (n, nx, nzm, ntr) of a block, another field per k"""
    shape, T, dt, _ = KINDS[name]
    return CM.make_s(shape[0] if n is None else n, shape[1], shape[2], T if ntr is None else ntr, dt, 500 + k)


def cell_add(M, p, name, s, c, mode, sl0=0, n=None, first=0, ntr=None, dsum=True, lead=None, call=None):
    """Plan.cell_add of a host s (n, nx, nzm, ntr) -> dsum (n, nzm, ntr) or None; s and the bands are checked.  call:
    another callable with Plan.cell_add's arguments (a shard plan's)."""
    import torch
    shape, T, dt, _ = KINDS[name]
    nx, nz = shape[1], shape[2]
    n = shape[0] - sl0 if n is None else n
    ntr = T - first if ntr is None else ntr
    assert s.shape == (n, nx, nz - 1, ntr) and s.dtype == dt
    lead = (ntr != 1) if lead is None else lead
    sh = M.cell_add_shapes(n, nx, nz, ntr if lead else None)
    sraw, sview = nan_banded(s, sh["s"])
    sorig = sraw.clone()
    buf = nan_out(sh["dsum"], dt) if dsum else None
    torch.cuda.synchronize()      # (the plan may run on a stream that does not wait for the one that filled the buffers)
    (call or p.cell_add)(sview, c, mode, buf[2] if buf else None, sl0, n, first, ntr)
    p.sync()
    torch.cuda.synchronize()
    assert torch.equal(sraw.view(torch.uint8), sorig.view(torch.uint8)), "s changed"
    if not buf:
        return None
    raw, pristine, view = buf
    assert torch.equal(raw[:BAND], pristine[:BAND]) and torch.equal(raw[-BAND:], pristine[-BAND:]), "dsum: a band byte changed"
    return to_host(view).reshape((n, nz - 1, ntr), order="F")


def model_add(m, name, s, c, mode, sl0=0, n=None, first=0, ntr=None):
    """the call on the plan model -> dsum; under CLIP the clip condition is asserted first"""
    ncrms, T = m.dims[0], m.dims[3]
    n = ncrms - sl0 if n is None else n
    ntr = T - first if ntr is None else ntr
    if mode == CLIP:
        frac = CM.clipped_fraction(m.a["f"][sl0:sl0 + n, ..., first:first + ntr], s, c)
        assert 0.1 <= frac <= 0.9, (name, sl0, n, first, ntr, frac)
    d = m.cell_add(s, c, mode, sl0=sl0, n=n, first=first, ntr=ntr)
    assert not isinstance(d, int), d
    return d


def snap(m):
    return {k: np.array(v, order="F") for k, v in m.export_device().items()}


def same(got, want, what):
    for k in ("f", "flux"):
        assert_bitwise(got[k], want[k], f"{what}: {k}")


# ---- 1. every kind of plan: whole plan, both modes, with and without dsum, every state, a run behind every call
# the script: (mode, dsum, k of s); the first behind the upload, the others behind a run (a windowed plan's seams are stale)
SCRIPT = ((ADD, True, 0), (CLIP, True, 1), (ADD, False, 2), (CLIP, False, 3))


@pytest.mark.parametrize("name", list(KINDS))
def test_every_plan_kind(mpdata, oracle, name):
    M = mpdata
    shape, T, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    c = factor(name)
    inp = inputs(oracle, name)
    F0 = inp["f"].reshape((ncrms, nx + 6, nz - 1, T), order="F")
    assert (F0 < 0).any() and (F0 > 0).any()
    # ---- the model's pass
    m = model_of(oracle, name)
    want = []
    for mode, dsum, k in SCRIPT:
        s = s_of(name, k)
        assert (s < 0).any() and (s > 0).any()
        before = np.array(m.a["f"], order="F")
        d = model_add(m, name, s, c, mode)
        new_f, new_d = CM.cell_add(before, s, c, mode)
        assert_bitwise(m.a["f"], new_f, "the plan model is the operator")
        assert_bitwise(d, new_d, "the plan model's dsum")
        assert_bitwise(new_f[:, :3], before[:, :3], "the halos stay")
        assert_bitwise(new_f[:, nx + 3:], before[:, nx + 3:], "the halos stay")
        assert not np.array_equal(new_f, before)
        after_call = snap(m)
        assert m.run() is None
        want.append((d, after_call, snap(m)))
    per = []
    if name in PERIODIC:
        assert m.set_boundary(PM.PERIODIC) is None
        assert m.run() is None
        for k, mode in ((5, CLIP), (6, ADD), (7, CLIP), (8, ADD)):
            s = s_of(name, k)
            d = model_add(m, name, s, c, mode)
            if k == 7:
                assert m.run() is None
            if k == 8:
                assert m.set_boundary(PM.GIVEN) is None
            per.append((d, snap(m)))
    # ---- the plan's pass
    p = new_plan(M, name)
    upload(p, inp)
    for (mode, dsum, k), (wd, w_call, w_run) in zip(SCRIPT, want):
        got = cell_add(M, p, name, s_of(name, k), c, mode, dsum=dsum)
        if dsum:
            assert_bitwise(got, wd, f"{name} script {k}: dsum")
        same(whole(M, p, name), w_call, f"{name} script {k} (mode {mode}, dsum {dsum}): the call")
        # a run on the kept velocities = export -> model -> import -> run: seams and the phantom are consistent
        p.run()
        same(whole(M, p, name), w_run, f"{name} script {k} (mode {mode}, dsum {dsum}): the call, run")
    if name in PERIODIC:
        p.set_boundary(M.BOUNDARY_PERIODIC)
        p.run()
        # (5) the halos are stale behind the run; the export hands out wrapped halos of the NEW field
        # (6) on halos the export just wrapped: they are copies of the OLD field now, the next export wraps again
        # (7) a run right behind the call, no read-back between   (8) back to GIVEN behind a call: the plan holds what an
        # export just before the switch would have returned
        for (k, mode), (wd, w) in zip(((5, CLIP), (6, ADD), (7, CLIP), (8, ADD)), per):
            got = cell_add(M, p, name, s_of(name, k), c, mode, dsum=k != 7)
            if got is not None:
                assert_bitwise(got, wd, f"{name} periodic {k}: dsum")
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
        s0 = s_of(name, 0)
        assert_bitwise(cell_add(M, p, name, s0, c, ADD), want[0][0], f"{name} FAST: dsum")
        assert_bitwise(whole(M, p, name, ("f",))["f"], want[0][1]["f"], f"{name} FAST upload, cell_add")
        p.run()
        E = whole(M, p, name, ("f",))["f"]
        s1 = s_of(name, 1)
        frac = CM.clipped_fraction(E, s1, c)
        assert 0.1 <= frac <= 0.9, frac
        got = cell_add(M, p, name, s1, c, CLIP)
        want_E, d_E = CM.cell_add(E, s1, c, CLIP)
        assert_bitwise(got, d_E, f"{name} FAST run, cell_add: dsum")
        assert_bitwise(whole(M, p, name, ("f",))["f"], want_E, f"{name} FAST run, cell_add")
        p.close()


# ---- 2. blocks and tracer sub-ranges: what lies outside keeps every bit
BLOCKS = {
    # eight instances per tile, five instances: inside the tile, one instance, the last one
    "f64-nz8": [(1, 3), (2, 1), (4, 1), (0, 5)],
    # two per tile: mid-tile to mid-tile, the last (half-filled) tile
    "f64-nz28-nx11": [(1, 3), (4, 1), (0, 4)],
    # three groups: a block that straddles a group boundary, odd sl0 across two boundaries, the last instance alone
    "f64-nz28-3groups": [(G - 1, 3), (3, 2 * G), (2 * G + 4, 1), (G, G)],
    "f64-nz72": [(1, 1), (1, 2)],
    "f64-nz140": [(1, 1), (0, 1)],
    # fp32 pairs: a block that splits pairs at both ends
    "f32-nz28-even": [(1, 3), (5, 1), (2, 2)],
    # 2G+3 pairs: across a group boundary (2G instances per group), splitting pairs
    "f32-nz28-3groups": [(2 * G - 1, 3), (1, 4 * G + 4), (4 * G + 5, 1)],
    # fp32 pairs, odd plan of 7 (instance 6 shares its pair with the phantom): blocks that hold and miss instance 6
    "f32-nz28-odd": [(1, 2), (6, 1), (5, 2), (0, 6), (3, 3), (0, 7)],
    "f32-nz72-odd": [(2, 1), (1, 1), (0, 2)],
    "f32-nz12-odd-ref": [(1, 3), (6, 1)],
    "f64-nz12-ref": [(1, 3), (4, 1)],
    # windowed plans: each behind an import (the first) and behind a run (the others: stale seams), a block and the whole
    "f64-nz239-tall": [(1, 1), (0, 1), (0, 2)],
    "f64-nz239-tall-2groups": [(G - 1, 3), (G + 1, 1), (1, G)],
    "f32-nz239-tall-odd": [(1, 1), (2, 1), (0, 2), (0, 3)],
}
# the first block of these splits an fp32 pair at one end at least: the instances next to it, the partner among them,
# hold -0.0 and negative values
SPLIT = {"f32-nz28-even": (0, 4), "f32-nz28-3groups": (2 * G - 2, 2 * G + 2), "f32-nz28-odd": (0, 3)}
# the windowed fp32 kind (its pairs are windows: with an odd number of windows a pair holds the last window of one instance
# and the first of the next) takes its -0.0 by a block import behind the last run and is read back without another run:
# where an input holds -0.0, the run of a windowed fp32 plan may return +0.0 on a level on which the tall model keeps -0.0
# (seen at one level of one instance; nothing of this call is involved), so no run follows a -0.0 here
SPLIT_TALL = {"f32-nz239-tall-odd": ((0, 2), (1, 1))}


@pytest.mark.parametrize("name", list(BLOCKS))
def test_blocks_leave_the_rest_alone(mpdata, oracle, name):
    """the modes alternate from CLIP; dsum on two calls of three.  Kinds of SPLIT: the uploaded f of the partner
    instances holds -0.0 on every second level of column 1 and negative values elsewhere, and the first call clips."""
    M = mpdata
    shape, T, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    c = factor(name)
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
        calls.append((k, sl0, n, first, ntr, CLIP if k % 2 == 0 else ADD, k % 3 != 2))
    # ---- the model's pass
    m = model_of(oracle, name, inp)
    want = []
    for k, sl0, n, first, ntr, mode, dsum in calls:
        before = snap(m)
        s = s_of(name, 10 + k, n, ntr)
        d = model_add(m, name, s, c, mode, sl0, n, first, ntr)
        after = snap(m)
        new = CM.cell_add(before["f"][sl0:sl0 + n, ..., first:first + ntr], s, c, mode)[0]
        assert_bitwise(after["f"][sl0:sl0 + n, ..., first:first + ntr], new, "inside")
        assert not np.array_equal(new, before["f"][sl0:sl0 + n, ..., first:first + ntr])
        assert m.run() is None
        want.append((d, before, after, snap(m)))
    # ---- the plan's pass
    p = new_plan(M, name)
    upload(p, inp)
    for (k, sl0, n, first, ntr, mode, dsum), (wd, w_before, w_after, w_run) in zip(calls, want):
        what = f"{name} block {sl0, n} tracers {first, ntr} mode {mode}"
        before = whole(M, p, name)
        same(before, w_before, what + ": before")
        got = cell_add(M, p, name, s_of(name, 10 + k, n, ntr), c, mode, sl0, n, first, ntr, dsum=dsum, lead=bool(k % 2) or ntr > 1)
        if dsum:
            assert_bitwise(got, wd, what + ": dsum")
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
            assert mode == CLIP
            for b in SPLIT[name]:
                assert out[b] and np.all(np.signbit(after["f"][b, 3, ::2, first]) & (after["f"][b, 3, ::2, first] == 0)), b
                assert (after["f"][b, 3:nx + 3, :, first] < 0).any(), b
        # a run of every instance (the phantom of an odd plan rides with instance ncrms - 1; a windowed plan refreshes
        # the seams the call marked stale; u, w, rho, rhow, adz enter it) matches the model
        p.run()
        same(whole(M, p, name), w_run, what + ": the call, run")
    if name in SPLIT_TALL:
        # stale seams behind the run; the neighbours take -0.0 by a block import, the block between them is clipped
        outside, (sl0, n) = SPLIT_TALL[name]
        for b in outside:
            fb = np.array(m.export_block(b, 1, ("f",), 0, T)["f"], order="F")
            fb[0, 3, ::2], fb[0, 4, ::2] = -0.0, -0.25
            p.import_block(b, f=to_dev(fb if T > 1 else fb[..., 0]))
            assert m.import_block(b, 1, {"f": fb}, 0, T) is None
        s = s_of(name, 19, n)
        wd = model_add(m, name, s, c, CLIP, sl0, n)
        assert_bitwise(cell_add(M, p, name, s, c, CLIP, sl0, n), wd, f"{name}: dsum beside -0.0")
        e = whole(M, p, name)
        same(e, snap(m), f"{name}: the call beside -0.0")
        for b in outside:
            assert np.all(np.signbit(e["f"][b, 3, ::2]) & (e["f"][b, 3, ::2] == 0)) and np.all(e["f"][b, 4, ::2] == -0.25), b
    p.close()


# ---- 3. the host form and the array forms
@pytest.mark.parametrize("name", ["f64-nz28-nx11", "f32-nz28-odd", "f64-nz12-ref", "f64-nz72", "f64-nz239-tall"])
def test_host_form(mpdata, oracle, name):
    M = mpdata
    shape, T, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    c = factor(name)
    tail = (T,) if T > 1 else ()
    script = ((0, ncrms, ADD, True), (1, 1, CLIP, False), (ncrms - 1, 1, ADD, True), (0, 2, CLIP, True))
    m = model_of(oracle, name)
    want = []
    for k, (sl0, n, mode, dsum) in enumerate(script):
        d = model_add(m, name, s_of(name, 20 + k, n), c, mode, sl0, n)
        after = snap(m)
        assert m.run() is None
        want.append((d, after, snap(m)))
    p = new_plan(M, name)
    upload(p, inputs(oracle, name))
    for k, ((sl0, n, mode, dsum), (wd, w_call, w_run)) in enumerate(zip(script, want)):
        s = s_of(name, 20 + k, n)
        sh = np.asfortranarray(s.reshape((n, nx, nz - 1) + tail, order="F"))
        keep = np.array(sh, order="F")
        d = np.full((n, nz - 1) + tail, np.nan, dt, order="F") if dsum else None
        p.cell_add_host(sh, c, mode, d, sl0, n)
        assert_bitwise(sh, keep, f"{name} host {sl0, n}: s")
        if d is not None:
            assert_bitwise(d.reshape(wd.shape, order="F"), wd, f"{name} host {sl0, n}: dsum")
        same(whole(M, p, name), w_call, f"{name} host form {sl0, n}")
        p.run()
        same(whole(M, p, name), w_run, f"{name} host form {sl0, n}, run")
    with pytest.raises(M.MpdataError):
        p.cell_add_host(sh[:, :, :-1], sl0=0, n=2)       # a wrong shape
    p.close()


# 257 and 600 instances: more than one block of 256 threads and a partly filled last one; (2, 1, 3) with 32769 tracers:
# 65538 rows, the second trip over gridDim.y.  f and s are random, so instance b differs from b - 256 and row r from
# r - 65535.  Each with a block inside the arrays.
ARRAYS = {"n257": ((257, 3, 6), 2, (1, 256)), "n600": ((600, 2, 5), 1, (300, 299)), "rows65538": ((2, 1, 3), 32769, (1, 1))}


@pytest.mark.parametrize("case", list(ARRAYS))
@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
def test_array_forms(mpdata, dt, case):
    import torch
    M = mpdata
    (ncrms, nx, nz), T, (b0, bn) = ARRAYS[case]
    rng = np.random.default_rng([77, ncrms, T])
    f = np.asfortranarray(rng.uniform(-0.5, 0.5, (ncrms, nx + 6, nz - 1, T)).astype(dt))
    c = 0.1 if dt == F32 else 0.75
    for (sl0, n), mode in (((0, ncrms), CLIP), ((b0, bn), ADD)):
        s = CM.make_s(n, nx, nz, T, dt, 600 + sl0)
        if mode == CLIP:
            assert 0.1 <= CM.clipped_fraction(f[sl0:sl0 + n], s, c) <= 0.9
        want, want_d = CM.cell_add(f[sl0:sl0 + n], s, c, mode)
        full = np.array(f, order="F")
        full[sl0:sl0 + n] = want
        if n > 256:
            assert not np.array_equal(want[256:], want[:n - 256]) and not np.array_equal(want_d[256:], want_d[:n - 256])
        if T > 32768:
            assert not np.array_equal(want[..., 32768:], want[..., :T - 32768])
        fd = to_dev(f)
        sh = M.cell_add_shapes(n, nx, nz, T)
        sraw, sview = nan_banded(s, sh["s"])
        sorig = sraw.clone()
        bd = nan_out(sh["dsum"], dt)
        torch.cuda.synchronize()
        M.cell_add(fd, sview, c, mode, bd[2], sl0, n)
        torch.cuda.synchronize()
        assert torch.equal(bd[0][:BAND], bd[1][:BAND]) and torch.equal(bd[0][-BAND:], bd[1][-BAND:])
        assert torch.equal(sraw.view(torch.uint8), sorig.view(torch.uint8)), "s changed"
        assert_bitwise(to_host(fd), full, f"array form {case} block {sl0, n}: f")
        assert_bitwise(to_host(bd[2]), want_d, f"array form {case} block {sl0, n}: dsum")
    if T == 1 or case == "n257":
        # one tracer without the tracer axis, dsum skipped
        f1 = to_dev(np.asfortranarray(f[..., 0]))
        s = CM.make_s(ncrms, nx, nz, None, dt, 650)
        M.cell_add(f1, to_dev(s), c)
        torch.cuda.synchronize()
        assert_bitwise(to_host(f1), CM.cell_add(f[..., 0], s, c)[0], f"array form {case}, one tracer: f")


# ---- 4. every error code, in the stated order; the plan's state before and after
def test_errors_change_nothing(mpdata, oracle):
    M = mpdata
    name = "f64-nz28-nx11"
    shape, T, dt, _ = KINDS[name]
    ncrms, nx, nz = shape
    inp = inputs(oracle, name)
    w = to_dev(s_of(name, 30))

    def code(fn, *a, **kw):
        with pytest.raises(M.MpdataError) as e:
            fn(*a, **kw)
        return e.value.code

    p = new_plan(M, name)
    assert code(p.cell_add, w) == M.ESTATE                                       # never filled
    upload(p, inp)
    before = whole(M, p, name)
    L = M.lib()
    raw = lambda sl0, n, first, ntr, s=w.data_ptr(), mode=0: L.mpdata_plan_cell_add_device(p._p, sl0, n, s, 0.75, mode, None, first, ntr)
    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, ncrms + 1), (ncrms, 1), (3, 3)):
        assert raw(sl0, n, 0, 1) == M.EINVAL, (sl0, n)
    for first, ntr in ((0, 0), (-1, 1), (1, 2), (2, 1), (0, 3)):
        assert raw(0, ncrms, first, ntr) == M.EINVAL, (first, ntr)
    assert raw(0, ncrms, 0, 1, None) == M.EINVAL and b"null s" in L.mpdata_last_error()
    for mode in (2, -1):
        assert raw(0, ncrms, 0, 1, mode=mode) == M.EINVAL and b"unknown mode" in L.mpdata_last_error()
    assert raw(0, ncrms, 0, 1, None, 2) == M.EINVAL and b"null s" in L.mpdata_last_error()        # the NULL before the mode
    assert raw(0, 0, 0, 1, None) == M.EINVAL and b"n = 0" in L.mpdata_last_error()                # the range first
    assert raw(0, ncrms, 0, 3, None) == M.EINVAL and b"tracer range" in L.mpdata_last_error()     # then the tracers
    assert code(p.cell_add, w, 0.75, 2) == M.EINVAL
    # a host form of the other precision; its NULL and its mode come first
    s32 = np.asfortranarray(s_of(name, 30).astype(F32))
    assert L.mpdata_plan_cell_add_f32(p._p, 0, ncrms, s32.ctypes.data, 0.75, 0, None) == M.ESTATE
    assert L.mpdata_plan_cell_add_f32(p._p, 0, ncrms, None, 0.75, 0, None) == M.EINVAL and b"null s" in L.mpdata_last_error()
    assert L.mpdata_plan_cell_add_f32(p._p, 0, ncrms, s32.ctypes.data, 0.75, 2, None) == M.EINVAL
    # the array forms: sizes, the block, f, then s, then the mode
    one = 8
    arr = L.mpdata_cell_add_device
    assert arr(4, 5, 1, 1, 0, 4, None, None, 0.75, 0, None, None) == M.EINVAL and b"nz=1" in L.mpdata_last_error()
    assert arr(4, 5, 6, 1, 2, 3, None, None, 0.75, 0, None, None) == M.EINVAL and b"outside" in L.mpdata_last_error()
    assert arr(4, 5, 6, 1, 0, 4, None, one, 0.75, 0, None, None) == M.EINVAL and b"null f" in L.mpdata_last_error()
    assert arr(4, 5, 6, 1, 0, 4, one, None, 0.75, 2, None, None) == M.EINVAL and b"null s" in L.mpdata_last_error()
    assert arr(4, 5, 6, 1, 0, 4, one, one, 0.75, 2, None, None) == M.EINVAL and b"unknown mode" in L.mpdata_last_error()
    after = whole(M, p, name)
    for k in before:
        assert_bitwise(after[k], before[k], f"after the refused calls: {k}")
    p.cell_add(w)                                                                # ... and the plan still works
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
    w = s_of(name, 40)
    with pytest.raises(M.MpdataError) as e:
        p.cell_add(to_dev(w))
    assert e.value.code == M.EUNSUPPORTED and b"mpdata_plan_shard_plan" in M.lib().mpdata_last_error()
    with pytest.raises(M.MpdataError) as e:
        p.cell_add_host(w)
    assert e.value.code == M.EUNSUPPORTED
    same(whole(M, p, name), m.export_device(), "after the refused handle calls")
    for g, (_, s0, nloc) in enumerate(p.shards()):
        q = p.shard_plan(g)
        sg = s_of(name, 41 + g, nloc)
        want = model_add(m, name, sg, 0.75, CLIP, s0, nloc)
        got = cell_add(M, q, name, sg, 0.75, CLIP, 0, nloc, call=q.cell_add)
        assert_bitwise(got, want, f"shard {g}: dsum")
        q.close()
    same(whole(M, p, name), m.export_device(), "after the shard plans' calls")
    p.run()
    assert m.run() is None
    same(whole(M, p, name), m.export_device(), "after the shard plans' calls and a run")
    p.close()


# ---- 6. the Fortran program: every record of its dump against the model
FORTRAN = {
    "f64": (F64, "cell_add_calls", (7, 5, 10), 3, (2, 3), (1, 2)), "f32": (F32, "cell_add_calls_sp", (6, 5, 10), 3, (1, 3), (1, 2)),
    "f64-whole": (F64, "cell_add_calls", (5, 3, 28), 2, (0, 5), (0, 2)), "f32-odd-ref": (F32, "cell_add_calls_sp", (7, 3, 12), 2, (6, 1), (1, 1)),
    "f64-nz72": (F64, "cell_add_calls", (3, 2, 72), 1, (1, 2), (0, 1)), "f32-nz72": (F32, "cell_add_calls_sp", (4, 2, 72), 2, (1, 2), (0, 2)),
}


@pytest.mark.parametrize("case", list(FORTRAN))
def test_fortran_program_matches_the_model(oracle, tmp_path, case):
    """the program's factors: 0.75 clipped on the block, 0.1 (a double; the fp32 program's plan rounds it once) on the range"""
    dt, exe, shape, T, (sl0, n), (t1, tn) = FORTRAN[case]
    ncrms, nx, nz = shape
    inp = CM.make_plan_inputs(oracle, shape, T, dt, SEED + 3)
    arrs = {k: (inp[k].reshape(inp[k].shape + (1,), order="F") if T == 1 and k in ("f", "flux") else inp[k]) for k in PM.NAMES}
    s_a = CM.make_s(n, nx, nz, T, dt, 700)
    s_b = CM.make_s(ncrms, nx, nz, tn, dt, 701)
    records = [("params", np.array([ncrms, nx, nz, T, sl0, n, t1, tn], np.int64))]
    records += [(k, arrs[k]) for k in PM.NAMES] + [("s_a", s_a), ("s_b", s_b)]
    # the replay on the model
    m = CM.PlanModelCellAdd(oracle, ncrms, nx, nz, T, dt)
    want = FR.want_import(m, inp)
    rc = lambda what, code=None: want.append(FR.rc(what, code))
    dsum = model_add(m, case, s_a, 0.75, CLIP, sl0, n)
    rc("add_block"); rc("sync")
    want += [("dsum", dsum)]
    assert not isinstance(m.cell_add(s_b, 0.1, ADD, first=t1, ntr=tn), int)
    rc("add_range"); rc("sync")
    want += FR.want_close(m)
    FR.compare_dump(FR.run_program(exe, records, tmp_path), want, case)
