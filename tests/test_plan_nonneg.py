"""GPU tests of the conservative per-level non-negativity fixer of a resident plan's tracers (include/mpdata_hip.h 3x):
mpdata_plan_nonneg_device, the host forms, the array forms, their Python face Plan.nonneg / nonneg_host / nonneg, and the
Fortran program tests/fortran/nonneg_calls.F90.

Every comparison is bit for bit (util.assert_bitwise) against the numpy model of tests/nonneg_model.py: NM.nonneg on a
reference-layout truth, or the plan model with the new call (Model below: an EXACT plan's f and flux are bit-identical to
it); behind a RUN of a field that holds -0.0 zeros are compared as zeros (same(), run=True).  sum and nneg are filled with NaN and lie between two patterned bands of 4 KiB, which must come back unchanged.  The
field is NM.make_field's: keep rows (no negative cell, some with a -0.0), fix rows (a negative cell, a positive sum) and
zero rows (a negative cell, no positive sum) on every level, negative values in the halo columns; before every call the
test asserts ON THE MODEL that the rows the call touches hold all three kinds (a row of nx = 1 cannot be a fix row), so
the early return and both branches of the update run.  u and w have no export: that they keep their bits shows in the run
behind the calls, which is compared with the model's.

Shapes (ncrms, nx, nz), the smallest at which a path of the kernels differs (NB = 8 columns in flight, KEPT up to nx = 32):
  (5, 4, 28)       wave-major fp64, two instances per tile and a half-filled last tile, one short batch
  (3, 1, 12)       one column
  (3, 31, 12), (3, 32, 12), (3, 33, 12)   the last short group of the KEPT form, its bound, and the RE-READ form (five
                   batches, the last of one column); (3, 33, 12) fp32 odd: the RE-READ form on pairs with the phantom
  (4, 3, 72), (3, 3, 72) fp32   pairs; odd with the switch (the phantom); (3, 3, 12) odd without it: the reference layout
  (3, 3, 65), (2, 3, 90)        the tail-wave layouts: element 63 | 64 across two slices
  (2, 3, 239) fp64, (3, 3, 300) fp32 odd   windowed plans, the second with an inner phantom
  (5, 3, 12) ref   a reference-layout plan
  (3, 4, 12) T = 5 a sub-range of three tracers"""
import numpy as np
import pytest

import fortran_records as FR
import level_add_model as AM
import level_stats_model as LM
import nonneg_model as NM
import plan_harness as H
from oracle import plan_model as PM
from plan_harness import _defaults, bands_kept, nan_out, upload
from util import assert_bitwise, to_dev, to_host

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32

# name -> (shape, tracers, dtype, switches)
KINDS = {
    "f64-nz28": ((5, 4, 28), 2, F64, {}), "f64-nx1": ((3, 1, 12), 1, F64, {}),
    "f64-nx31": ((3, 31, 12), 1, F64, {}), "f64-nx32": ((3, 32, 12), 2, F64, {}), "f64-nx33": ((3, 33, 12), 2, F64, {}),
    "f32-nz72-even": ((4, 3, 72), 2, F32, {}), "f32-nz72-odd": ((3, 3, 72), 2, F32, dict(odd=True)),
    "f32-nz12-odd-ref": ((3, 3, 12), 1, F32, {}),     # (an odd fp32 plan without the switch keeps the reference layout)
    "f32-nx32-odd": ((3, 32, 12), 1, F32, dict(odd=True)), "f32-nx33-odd": ((3, 33, 12), 2, F32, dict(odd=True)),
    "f64-nz65": ((3, 3, 65), 1, F64, {}), "f64-nz90": ((2, 3, 90), 1, F64, {}),
    "f64-nz239-tall": ((2, 3, 239), 2, F64, dict(tall=True)), "f32-nz300-tall-odd": ((3, 3, 300), 1, F32, dict(tall=True, odd=True)),
    "f64-nz12-ref": ((5, 3, 12), 2, F64, dict(ref=True)),
    "f64-nz12-T5": ((3, 4, 12), 5, F64, {}),
}
REF = ("f32-nz12-odd-ref", "f64-nz12-ref")
FAST = ("f64-nz28", "f64-nx33", "f32-nz72-odd", "f64-nz12-ref", "f64-nz239-tall")
PERIODIC = ("f64-nz28", "f64-nx33", "f32-nz72-odd", "f64-nz12-ref", "f32-nz300-tall-odd")
SEED = 100


class Model(AM.PlanModelAdd, NM.PlanModelNonneg):
    pass


_INPUTS = {}


def inputs(oracle, name):
    """the seven arrays of KINDS[name]: computed once and shared; no test writes them"""
    if name not in _INPUTS:
        shape, T, dt, _ = KINDS[name]
        _INPUTS[name] = NM.make_plan_inputs(oracle, shape, T, dt, SEED)
    return _INPUTS[name]


def new_plan(M, name, variant=None):
    return H.new_plan(M, KINDS[name], name, name in REF, bool(KINDS[name][3].get("tall")), variant)


def model_of(oracle, name, inp=None):
    shape, T, dt, _ = KINDS[name]
    m = Model(oracle, *shape, T, dt)
    assert m.upload({k: np.array(v, order="F") for k, v in (inp or inputs(oracle, name)).items()}) is None
    return m


def whole(M, p, name, what=("f", "flux")):
    return H.whole(M, p, KINDS[name], what)


def nonneg(M, p, name, sl0=0, n=None, first=0, ntr=None, want=("sum", "nneg"), lead=None, call=None):
    """Plan.nonneg -> {name: host array (n, nzm, ntr)} of the outputs asked for; the bands are checked.  call: another
    callable with Plan.nonneg's arguments (a shard plan's)."""
    import torch
    shape, T, dt, _ = KINDS[name]
    nx, nz = shape[1], shape[2]
    n = shape[0] - sl0 if n is None else n
    ntr = T - first if ntr is None else ntr
    lead = (ntr != 1) if lead is None else lead
    sh = M.nonneg_shapes(n, nx, nz, ntr if lead else None)
    bufs = {k: nan_out(sh[k], dt) for k in want}
    torch.cuda.synchronize()      # (the plan may run on a stream that does not wait for the one that filled the buffers)
    (call or p.nonneg)(bufs["sum"][2] if "sum" in bufs else None, bufs["nneg"][2] if "nneg" in bufs else None, sl0, n, first, ntr)
    p.sync()
    torch.cuda.synchronize()
    out = {}
    for k, (raw, pristine, view) in bufs.items():
        assert bands_kept(raw, pristine), f"{k}: a band byte changed"
        out[k] = to_host(view).reshape((n, nz - 1, ntr), order="F")
    return out


def model_nonneg(m, name, sl0=0, n=None, first=0, ntr=None, kinds=True):
    """the call on the plan model -> {sum, nneg}; that the rows it touches hold every kind is asserted first"""
    if kinds:
        assert NM.has_all_kinds(m.a["f"], sl0, n, first, ntr), (name, sl0, n, first, ntr)
    r = m.nonneg(sl0=sl0, n=n, first=first, ntr=ntr)
    assert not isinstance(r, int), r
    return {"sum": r[0], "nneg": r[1]}


def incr(name, k):
    """d (ncrms, nzm, T) of a level_add that leaves rows of every kind behind a run: another increment per instance, level
    and tracer, most of them below zero"""
    shape, T, dt, _ = KINDS[name]
    rng = np.random.default_rng([SEED, k, shape[0], shape[2], T])
    return np.asfortranarray(rng.uniform(-0.7, 0.2, (shape[0], shape[2] - 1, T)).astype(dt))


def dirty(p, name, k):
    d = incr(name, k)
    p.level_add(to_dev(d if KINDS[name][1] > 1 else d[..., 0]))


def snap(m):
    return {k: np.array(v, order="F") for k, v in m.export_device().items()}


def same(got, want, what, run=False):
    """bit for bit.  run: the comparison stands behind a run of a field that holds -0.0 (the keep rows keep theirs) -- there
    a zero may come out of the advection kernels with the other sign than the oracle's (the table of section 1:
    the hardware max / min order -0 below +0), which is no matter of this call: zeros are compared as zeros"""
    for k in ("f", "flux"):
        g, w = (AM.canon(got[k]), AM.canon(want[k])) if run else (got[k], want[k])
        assert_bitwise(g, w, f"{what}: {k}")


# ---- 1. every kind of plan: the whole plan behind the upload, behind a run and a level_add (a windowed plan's seams are
# stale), each output absent in turn, a second call right behind the first, a run behind the calls
SCRIPT = (("sum", "nneg"), ("sum",), ("nneg",))


@pytest.mark.parametrize("name", list(KINDS))
def test_every_plan_kind(mpdata, oracle, name):
    M = mpdata
    shape, T, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    inp = inputs(oracle, name)
    # ---- the model's pass
    m = model_of(oracle, name)
    want = []
    for k, outs in enumerate(SCRIPT):
        before = np.array(m.a["f"], order="F")
        o = model_nonneg(m, name)
        new_f, new_s, new_c = NM.nonneg(before)
        assert_bitwise(m.a["f"], new_f, "the plan model is the operator")
        assert_bitwise(o["sum"], new_s, "the plan model's sum")
        assert_bitwise(o["sum"], LM.level_stats(before)[0], "the sum of level_stats")
        assert_bitwise(new_f[:, :3], before[:, :3], "the halos stay")
        assert_bitwise(new_f[:, nx + 3:], before[:, nx + 3:], "the halos stay")
        after_call = snap(m)
        again = model_nonneg(m, name, kinds=False)
        assert not again["nneg"].any()
        assert_bitwise(m.export_device()["f"], after_call["f"], "idempotent")
        assert m.run() is None
        want.append((o, after_call, again, snap(m)))
        assert m.level_add(incr(name, 10 + k)) is None
    per = []
    if name in PERIODIC:
        assert m.set_boundary(PM.PERIODIC) is None
        assert m.run() is None
        for k in (20, 21):
            assert m.level_add(incr(name, k)) is None
            o = model_nonneg(m, name)
            if k == 21:
                assert m.run() is None
            per.append((o, snap(m)))
    # ---- the plan's pass
    p = new_plan(M, name)
    upload(p, inp)
    for k, (outs, (wo, w_call, w_again, w_run)) in enumerate(zip(SCRIPT, want)):
        got = nonneg(M, p, name, want=outs)
        for o in outs:
            assert_bitwise(got[o], wo[o], f"{name} script {k}: {o}")
        same(whole(M, p, name), w_call, f"{name} script {k} ({outs}): the call")
        # the second call finds nothing to fix: nneg == 0, the sums of the new field, every bit kept
        got = nonneg(M, p, name, want=("sum", "nneg") if k == 0 else ())
        if k == 0:
            assert not got["nneg"].any()
            assert_bitwise(got["sum"], w_again["sum"], f"{name} script {k}: the second call's sum")
        same(whole(M, p, name), w_call, f"{name} script {k}: the second call")
        # a run on the kept velocities = export -> model -> import -> run: seams and the phantom are consistent
        p.run()
        same(whole(M, p, name), w_run, f"{name} script {k} ({outs}): the call, run", run=True)
        dirty(p, name, 10 + k)
    if name in PERIODIC:
        p.set_boundary(M.BOUNDARY_PERIODIC)
        p.run()
        # (20) the halos are stale behind the run and the level_add; the export hands out wrapped halos of the NEW field
        # (21) a run right behind the call, no read-back between
        for k, (wo, w) in zip((20, 21), per):
            dirty(p, name, k)
            got = nonneg(M, p, name)
            for o in got:
                assert_bitwise(got[o], wo[o], f"{name} periodic {k}: {o}")
            if k == 21:
                p.run()
            e = whole(M, p, name)
            same(e, w, f"{name} periodic {k}", run=k == 21)
            if k == 20:
                assert_bitwise(e["f"], PM.wrap(np.array(e["f"], order="F")), f"{name} periodic {k}: the halos are wrapped copies of the new interior")
                assert np.all(e["f"] >= 0) and not np.signbit(e["f"][:, 3:nx + 3]).any()
    p.close()
    if name in FAST:
        # FAST: the same bits as EXACT on the uploaded f -- nothing of the call is contracted
        p = new_plan(M, name, variant=M.VARIANT_FAST)
        upload(p, inp)
        got = nonneg(M, p, name)
        for o in got:
            assert_bitwise(got[o], want[0][0][o], f"{name} FAST: {o}")
        assert_bitwise(whole(M, p, name, ("f",))["f"], want[0][1]["f"], f"{name} FAST upload, nonneg")
        p.close()


# ---- 2. blocks and tracer sub-ranges: what lies outside keeps every bit.  (sl0, n, first, ntr); None: all tracers
BLOCKS = {
    # two per tile: mid-tile to mid-tile, the last (half-filled) tile, one instance
    "f64-nz28": [(1, 3, 0, 1), (4, 1, 1, 1), (0, 4, 0, 2), (2, 1, 0, 2)],
    "f64-nx32": [(1, 1, 1, 1), (0, 2, 0, 2)], "f64-nx33": [(1, 1, 0, 1), (1, 2, 0, 2)],
    # fp32 pairs: a block that splits pairs at both ends, at one end, a whole pair
    "f32-nz72-even": [(1, 2, 0, 1), (3, 1, 1, 1), (0, 1, 0, 2), (2, 2, 0, 2)],
    # fp32 pairs, odd plan of 3 (instance 2 shares its pair with the phantom): blocks that hold and miss instance 2
    "f32-nz72-odd": [(1, 1, 0, 1), (2, 1, 1, 1), (1, 2, 0, 2), (0, 2, 0, 2), (0, 3, 0, 2)],
    "f32-nx33-odd": [(1, 1, 0, 1), (2, 1, 1, 1), (0, 1, 0, 2), (0, 3, 0, 2)],
    "f32-nx32-odd": [(1, 1, 0, 1), (2, 1, 0, 1), (0, 2, 0, 1)],
    "f32-nz12-odd-ref": [(1, 1, 0, 1), (2, 1, 0, 1)],
    "f64-nz65": [(1, 1, 0, 1), (1, 2, 0, 1)], "f64-nz90": [(1, 1, 0, 1), (0, 1, 0, 1)],
    "f64-nz12-ref": [(1, 3, 1, 1), (4, 1, 0, 2)],
    "f64-nz239-tall": [(1, 1, 0, 1), (0, 1, 1, 1), (0, 2, 0, 2)],
    "f32-nz300-tall-odd": [(1, 1, 0, 1), (2, 1, 0, 1), (0, 2, 0, 1), (0, 3, 0, 1)],
    # a sub-range of three tracers of five: the first, the last and the rest keep every bit
    "f64-nz12-T5": [(0, 3, 1, 3), (1, 2, 2, 3), (1, 1, 0, 3)],
}
# the first block of these splits an fp32 pair at one end at least: the instances next to it, the partner among them,
# hold -0.0 and negative values on rows of their own
SPLIT = {"f32-nz72-even": (0, 3), "f32-nz72-odd": (0,), "f32-nx33-odd": (0,), "f32-nx32-odd": (0,), "f32-nz300-tall-odd": (0,)}


@pytest.mark.parametrize("name", list(BLOCKS))
def test_blocks_leave_the_rest_alone(mpdata, oracle, name):
    """before every call but the first the whole plan takes a fresh field of every kind by an import of f.  Kinds of
    SPLIT: the uploaded f of the partner instances holds -0.0 on every second level of column 1 and a negative value
    beside it."""
    M = mpdata
    shape, T, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    inp = dict(inputs(oracle, name))
    if name in SPLIT:
        f = np.array(inp["f"], order="F")
        for b in SPLIT[name]:
            f[b, 3, ::2] = -0.0
            f[b, 3 + (nx > 1), 1::2] = -0.25
        inp["f"] = f
    fresh = lambda k: NM.make_field(ncrms, nx, nz, None if T == 1 else T, dt, SEED + 50 + k)
    # ---- the model's pass
    m = model_of(oracle, name, inp)
    want = []
    for k, (sl0, n, first, ntr) in enumerate(BLOCKS[name]):
        if k:
            assert m.import_device({"f": fresh(k)}) is None
        before = snap(m)
        o = model_nonneg(m, name, sl0, n, first, ntr)
        after = snap(m)
        new = NM.nonneg(before["f"][sl0:sl0 + n, ..., first:first + ntr])[0]
        assert_bitwise(after["f"][sl0:sl0 + n, ..., first:first + ntr], new, "inside")
        assert not np.array_equal(after["f"], before["f"])
        want.append((o, before, after))
    assert m.nonneg() is not None and m.run() is None
    w_run = snap(m)
    # ---- the plan's pass
    p = new_plan(M, name)
    upload(p, inp)
    for k, ((sl0, n, first, ntr), (wo, w_before, w_after)) in enumerate(zip(BLOCKS[name], want)):
        what = f"{name} block {sl0, n} tracers {first, ntr}"
        if k:
            p.import_device(f=to_dev(fresh(k)))
        before = whole(M, p, name)
        same(before, w_before, what + ": before")
        outs = (("sum", "nneg"), ("nneg",), ("sum",))[k % 3]
        got = nonneg(M, p, name, sl0, n, first, ntr, want=outs, lead=bool(k % 2) or ntr > 1)
        for o in outs:
            assert_bitwise(got[o], wo[o], what + ": " + o)
        after = whole(M, p, name)
        out = np.ones(ncrms, bool)
        out[sl0:sl0 + n] = False
        tout = np.ones(T, bool)
        tout[first:first + ntr] = False
        assert_bitwise(after["f"][out], before["f"][out], what + ": instances outside")
        assert_bitwise(after["f"][..., tout], before["f"][..., tout], what + ": tracers outside")
        assert not out.any() or (before["f"][out][:, 3:nx + 3] < 0).any()          # (what lies outside has something to lose)
        assert not tout.any() or (before["f"][..., tout][:, 3:nx + 3] < 0).any()
        assert_bitwise(after["flux"], before["flux"], what + ": flux")
        same(after, w_after, what + ": the call")
        if k == 0 and name in SPLIT:
            for b in SPLIT[name]:
                assert out[b] and np.all(np.signbit(after["f"][b, 3, ::2, first]) & (after["f"][b, 3, ::2, first] == 0)), b
                assert np.all(after["f"][b, 3 + (nx > 1), 1::2, first] == -0.25), b
    # the rest of the plan fixed, then a run of every instance (the phantom of an odd plan rides with instance ncrms - 1; a
    # windowed plan refreshes the seams the calls marked stale; u, w, rho, rhow, adz enter it) matches the model
    p.nonneg()
    p.run()
    same(whole(M, p, name), w_run, f"{name}: the calls, run", run=True)
    p.close()


# ---- 3. a field without a negative cell: nothing is stored -- the export is bit-identical, -0.0 included, nneg is zero
@pytest.mark.parametrize("name", ["f64-nz28", "f64-nx32", "f64-nx33", "f32-nz72-odd", "f32-nx33-odd", "f64-nz12-ref", "f64-nz239-tall"])
def test_clean_field_keeps_every_bit(mpdata, oracle, name):
    M = mpdata
    shape, T, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    inp = dict(inputs(oracle, name))
    inp["f"] = f = NM.make_clean_field(ncrms, nx, nz, None if T == 1 else T, dt, SEED + 7)
    F = f.reshape(f.shape + (() if T > 1 else (1,)), order="F")
    assert not (F[:, 3:nx + 3] < 0).any() and (np.signbit(F[:, 3:nx + 3]) & (F[:, 3:nx + 3] == 0)).any()
    assert set(np.unique(NM.kinds(F)).tolist()) == {NM.KEEP}
    p = new_plan(M, name)
    upload(p, inp)
    before = whole(M, p, name)
    got = nonneg(M, p, name)
    assert not got["nneg"].any() and not np.signbit(got["nneg"]).any()
    assert_bitwise(got["sum"], LM.level_stats(F)[0], f"{name}: sum")
    after = whole(M, p, name)
    same(after, before, f"{name}: a clean field")
    assert_bitwise(after["f"], F, f"{name}: the uploaded field")
    p.close()


# ---- 4. the host form and the array forms
@pytest.mark.parametrize("name", ["f64-nz28", "f32-nz72-odd", "f64-nz12-ref", "f64-nz90", "f64-nz239-tall", "f64-nx33"])
def test_host_form(mpdata, oracle, name):
    M = mpdata
    shape, T, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    tail = (T,) if T > 1 else ()
    script = ((1, 1, ("sum", "nneg")), (ncrms - 1, 1, ("nneg",)), (0, ncrms, ("sum",)), (0, 2, ()))
    m = model_of(oracle, name)
    want = []
    for k, (sl0, n, outs) in enumerate(script):
        o = model_nonneg(m, name, sl0, n, kinds=k == 0 or (k == 1 and ncrms > 2))
        want.append((o, snap(m)))
    assert m.run() is None
    w_run = snap(m)
    p = new_plan(M, name)
    upload(p, inputs(oracle, name))
    for k, ((sl0, n, outs), (wo, w_call)) in enumerate(zip(script, want)):
        h = {o: np.full((n, nz - 1) + tail, np.nan, dt, order="F") for o in outs}
        p.nonneg_host(h.get("sum"), h.get("nneg"), sl0, n)
        for o in outs:
            assert_bitwise(h[o].reshape(wo[o].shape, order="F"), wo[o], f"{name} host {sl0, n}: {o}")
        same(whole(M, p, name), w_call, f"{name} host form {sl0, n}")
    p.run()
    same(whole(M, p, name), w_run, f"{name} host forms, run", run=True)
    with pytest.raises(M.MpdataError):
        p.nonneg_host(np.zeros((2, nz - 2) + tail, dt, order="F"), sl0=0, n=2)              # a wrong shape
    p.close()


# 257 instances: more than one block of 256 threads and a partly filled last one; (2, 1, 3) with 32769 tracers: 65538 rows,
# the second trip over gridDim.y; 33 columns: five batches of the walks.  Each with a block inside the arrays, sl0 > 0.
ARRAYS = {"n257": ((257, 3, 9), 2, (1, 256)), "nx33": ((6, 33, 9), 1, (2, 3)), "rows65538": ((2, 1, 3), 32769, (1, 1))}


@pytest.mark.parametrize("case", list(ARRAYS))
@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
def test_array_forms(mpdata, dt, case):
    import torch
    M = mpdata
    (ncrms, nx, nz), T, (b0, bn) = ARRAYS[case]
    if nz - 1 >= 7:
        f = NM.make_field(ncrms, nx, nz, T, dt, 77)
    else:                                                    # (two levels: the planted pattern needs seven)
        f = np.asfortranarray(np.random.default_rng([77, ncrms, T]).uniform(-0.5, 0.5, (ncrms, nx + 6, nz - 1, T)).astype(dt))
    for sl0, n in ((b0, bn), (0, ncrms)):
        assert NM.has_all_kinds(f, sl0, n)
        want, want_s, want_c = NM.nonneg(f[sl0:sl0 + n])
        full = np.array(f, order="F")
        full[sl0:sl0 + n] = want
        if n > 256:
            assert not np.array_equal(want[256:], want[:n - 256]) and not np.array_equal(want_s[256:], want_s[:n - 256])
        if T > 32768:
            assert not np.array_equal(want_s[..., 32768:], want_s[..., :T - 32768])
        fd = to_dev(f)
        sh = M.nonneg_shapes(n, nx, nz, T)
        bs, bc = nan_out(sh["sum"], dt), nan_out(sh["nneg"], dt)
        torch.cuda.synchronize()
        M.nonneg(fd, bs[2], bc[2], sl0, n)
        torch.cuda.synchronize()
        assert bands_kept(bs[0], bs[1]) and bands_kept(bc[0], bc[1])
        assert_bitwise(to_host(fd), full, f"array form {case} block {sl0, n}: f")
        assert_bitwise(to_host(bs[2]), want_s, f"array form {case} block {sl0, n}: sum")
        assert_bitwise(to_host(bc[2]), want_c, f"array form {case} block {sl0, n}: nneg")
    if case == "n257":
        # one tracer without the tracer axis, both outputs skipped
        f1 = to_dev(np.asfortranarray(f[..., 0]))
        M.nonneg(f1, sl0=3)
        torch.cuda.synchronize()
        full = np.array(f[..., 0], order="F")
        full[3:] = NM.nonneg(f[3:, ..., 0])[0]
        assert_bitwise(to_host(f1), full, f"array form {case}, one tracer: f")


# ---- 5. every error code, in the stated order; the plan's state before and after
def test_errors_change_nothing(mpdata, oracle):
    M = mpdata
    name = "f64-nz28"
    shape, T, dt, _ = KINDS[name]
    ncrms, nx, nz = shape
    inp = inputs(oracle, name)
    assert NM.has_all_kinds(inp["f"])

    def code(fn, *a, **kw):
        with pytest.raises(M.MpdataError) as e:
            fn(*a, **kw)
        return e.value.code

    p = new_plan(M, name)
    assert code(p.nonneg) == M.ESTATE                                            # never filled
    upload(p, inp)
    before = whole(M, p, name)
    L = M.lib()
    raw = lambda sl0, n, first, ntr: L.mpdata_plan_nonneg_device(p._p, sl0, n, None, None, first, ntr)
    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, ncrms + 1), (ncrms, 1), (3, 3)):
        assert raw(sl0, n, 0, 1) == M.EINVAL, (sl0, n)
    for first, ntr in ((0, 0), (-1, 1), (1, 2), (2, 1), (0, 3)):
        assert raw(0, ncrms, first, ntr) == M.EINVAL, (first, ntr)
    assert raw(0, 0, 0, 3) == M.EINVAL and b"n = 0" in L.mpdata_last_error()                      # the range first
    assert raw(0, ncrms, 0, 3) == M.EINVAL and b"tracer range" in L.mpdata_last_error()           # then the tracers
    # a host form of the other precision; the range comes first
    s32 = np.zeros((ncrms, nz - 1, T), F32, order="F")
    assert L.mpdata_plan_nonneg_f32(p._p, 0, ncrms, s32.ctypes.data, None) == M.ESTATE
    assert L.mpdata_plan_nonneg_f32(p._p, 0, 0, s32.ctypes.data, None) == M.EINVAL
    assert not s32.any()
    # the array forms: sizes, the block, then f
    arr = L.mpdata_nonneg_device
    assert arr(4, 5, 1, 1, 0, 4, None, None, None, None) == M.EINVAL and b"nz=1" in L.mpdata_last_error()
    assert arr(4, 5, 6, 1, 2, 3, None, None, None, None) == M.EINVAL and b"outside" in L.mpdata_last_error()
    assert arr(4, 5, 6, 1, 0, 4, None, None, None, None) == M.EINVAL and b"null f" in L.mpdata_last_error()
    after = whole(M, p, name)
    for k in before:
        assert_bitwise(after[k], before[k], f"after the refused calls: {k}")
    p.nonneg()                                                                   # ... and the plan still works, no output asked
    p.sync()
    assert_bitwise(whole(M, p, name, ("f",))["f"], NM.nonneg(before["f"])[0], "both outputs NULL")
    p.close()


# ---- 6. a multi-GPU handle is refused; the single-device plans of its shards take the call
def test_multi_gpu_handle_and_shard_plan(mpdata, oracle, monkeypatch):
    M = mpdata
    monkeypatch.delenv("MPDATA_MULTI_XFER", raising=False)
    name = "f64-nz28"
    shape, T, dt, _ = KINDS[name]
    inp = inputs(oracle, name)
    p = M.Plan(*shape, T, dtype=dt, devices=[0, 0])
    upload(p, inp)
    m = model_of(oracle, name)
    with pytest.raises(M.MpdataError) as e:
        p.nonneg()
    assert e.value.code == M.EUNSUPPORTED and b"mpdata_plan_shard_plan" in M.lib().mpdata_last_error()
    with pytest.raises(M.MpdataError) as e:
        p.nonneg_host()
    assert e.value.code == M.EUNSUPPORTED
    same(whole(M, p, name), m.export_device(), "after the refused handle calls")
    for g, (_, s0, nloc) in enumerate(p.shards()):
        q = p.shard_plan(g)
        want = model_nonneg(m, name, s0, nloc)
        got = nonneg(M, q, name, 0, nloc, call=q.nonneg)
        for o in got:
            assert_bitwise(got[o], want[o], f"shard {g}: {o}")
        q.close()
    same(whole(M, p, name), m.export_device(), "after the shard plans' calls")
    p.run()
    assert m.run() is None
    same(whole(M, p, name), m.export_device(), "after the shard plans' calls and a run", run=True)
    p.close()


# ---- 7. the Fortran program: every record of its dump against the model
FORTRAN = {
    "f64": (F64, "nonneg_calls", (7, 5, 10), 3, (2, 3), (1, 2)), "f32": (F32, "nonneg_calls_sp", (6, 5, 10), 3, (1, 3), (1, 2)),
    "f64-whole": (F64, "nonneg_calls", (5, 3, 28), 2, (0, 5), (0, 2)), "f32-odd-ref": (F32, "nonneg_calls_sp", (7, 3, 12), 2, (6, 1), (1, 1)),
    "f64-nz72": (F64, "nonneg_calls", (3, 2, 72), 1, (1, 2), (0, 1)), "f32-nz72": (F32, "nonneg_calls_sp", (4, 2, 72), 2, (1, 2), (0, 2)),
}


@pytest.mark.parametrize("case", list(FORTRAN))
def test_fortran_program_matches_the_model(oracle, tmp_path, case):
    """the program's calls: the device form on the block, all tracers; the device form on the whole plan, a tracer range,
    the sum alone; the host form on the whole plan, nneg alone; the array form on the block of the imported array; a
    refused call"""
    dt, exe, shape, T, (sl0, n), (t1, tn) = FORTRAN[case]
    ncrms, nx, nz = shape
    inp = NM.make_plan_inputs(oracle, shape, T, dt, SEED + 3)
    arrs = {k: (inp[k].reshape(inp[k].shape + (1,), order="F") if T == 1 and k in ("f", "flux") else inp[k]) for k in PM.NAMES}
    records = [("params", np.array([ncrms, nx, nz, T, sl0, n, t1, tn], np.int64))] + [(k, arrs[k]) for k in PM.NAMES]
    # the replay on the model
    m = Model(oracle, ncrms, nx, nz, T, dt)
    want = FR.want_import(m, inp)
    rc = lambda what, code=None: want.append(FR.rc(what, code))
    a = model_nonneg(m, case, sl0, n)
    rc("nonneg_block"); rc("sync")
    want += [("sum_a", a["sum"]), ("nneg_a", a["nneg"])]
    b = model_nonneg(m, case, 0, ncrms, t1, tn, kinds=False)
    rc("nonneg_range"); rc("sync")
    want += [("sum_b", b["sum"])]
    c = model_nonneg(m, case, kinds=False)
    assert n == ncrms or tn == T or c["nneg"].any()                     # (what the two calls before left to fix)
    rc("nonneg_host")
    want += [("nneg_c", c["nneg"])]
    f_arr = np.array(arrs["f"], order="F")
    f_arr[sl0:sl0 + n], s_d, c_d = NM.nonneg(arrs["f"][sl0:sl0 + n])
    rc("nonneg_array"); rc("dsync")
    want += [("sum_d", s_d), ("nneg_d", c_d), ("f_arr", f_arr)]
    rc("nonneg_none", m.nonneg(sl0=sl0, n=0))
    want += FR.want_close(m)
    got = FR.run_program(exe, records, tmp_path)
    assert [k for k, _ in got] == [k for k, _ in want]
    for (k, ga), (_, wa) in zip(got, want):
        wa = np.asfortranarray(wa).reshape(ga.shape, order="F")
        if k in ("f_e", "flux_e"):                           # behind the program's run: zeros as zeros (same(), run=True)
            ga, wa = AM.canon(ga), AM.canon(wa)
        assert_bitwise(ga, wa, f"{case}: record {k}")
