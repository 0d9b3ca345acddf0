"""GPU tests of the linear combinations of the tracers of a resident plan (include/mpdata_hip.h 3z):
mpdata_plan_combine_device, the host forms, the array forms, their Python face Plan.combine / combine_host / combine, and
the Fortran program tests/fortran/combine_calls.F90.

Every comparison is against the numpy model of tests/combine_model.py: CB.combine on a reference-layout truth, or the plan
model with the new call (CB.PlanModelCombine: an EXACT plan's f and flux are bit-identical to it), or, for FAST plans, the
plan's own whole export before the call.  The comparison is CB.same: bit for bit, but that a NaN of the model is met by any
NaN (the sign and payload of a NaN an operation returns are the processor's: tests/combine_model.py); the copy form, where
nothing is computed, is compared with util.assert_bitwise, NaN payloads included.  coef and c0 lie inside larger buffers
with 4 KiB of NaN on both sides, so a read outside the block's arrays poisons the result; sum is filled with NaN and lies
between two patterned bands of 4 KiB, which must come back unchanged, and so must coef and c0.

Two passes per kind.  (A) the field carries planted -0.0, +inf, -inf and NaNs with payloads of both signs in the interior of
every tracer (CB.plant_specials); the SCRIPT of calls runs on it without a run between -- every class of the source count
(0, 1, 2, 3 to 4, 5 to 8), dst below, above and among the sources, repeated sources, coef and c0 on and off, CLIP, sum on and
off -- and after each call the whole plan, every tracer and the halos, is compared with the model.  (B) on the clean field
(a run does not agree with the oracle on NaN) calls with a run behind each: seams, the phantom and u, w enter it.

Shapes (ncrms, nx, nz), the smallest at which a path of the kernel differs (8, 4, 3 or 2 columns in flight by the source
count and the precision): those of tests/test_plan_convert.py with four tracers -- nz 8 (padding slots); nz 28 with nx 8, 11, 17 (at, above
and twice above the columns in flight); nz 64, 65, 72, 140, 238 (one slice, several, idle lanes and waves); 37 fp64 and 74
fp32 instances (several workgroups); fp32 even and odd; the reference layout, nz 250 among it; windowed plans at nz 239 and
300, odd fp32 among them --, one kind of nine tracers (eight distinct sources and a ninth dst), and nx = 1 and 2 in both
precisions, where the walk clamps (no run: pass A alone)."""
import numpy as np
import pytest

import combine_model as CB
import convert_model as CV
import fortran_records as FR
import level_add_model as AM
import plan_harness as H
from oracle import plan_model as PM
from plan_harness import BAND, _defaults, nan_banded, nan_out, upload
from util import assert_bitwise, to_dev, to_host

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
T = 4

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
    "f64-nz8-T9": ((3, 3, 8), 9, F64, {}),
    "f64-nz28-nx1": ((3, 1, 28), T, F64, dict(norun=True)), "f64-nz28-nx2": ((3, 2, 28), T, F64, dict(norun=True)),
    "f32-nz28-nx1-odd": ((5, 1, 28), T, F32, dict(odd=True, norun=True)), "f32-nz28-nx2": ((6, 2, 28), T, F32, dict(norun=True)),
}
REF = ("f32-nz12-odd-ref", "f64-nz12-ref", "f32-nz12-ref", "f64-nz250-ref")
# one kind of each family runs the FAST variant too; five kinds run a PERIODIC plan
FAST = ("f64-nz28-nx11", "f64-nz72", "f32-nz28-odd", "f64-nz12-ref", "f64-nz239-tall")
PERIODIC = ("f64-nz28-nx11", "f32-nz72-odd", "f64-nz12-ref", "f32-nz239-tall-odd", "f64-nz28-nx17")
SEED = 100

# pass A: (dst, src, coef, c0, mode, sum).  The first is the copy, right behind the upload: compared bit for bit.
SCRIPT = ((3, (1,), False, False, 0, True),                       # one source: the copy, dst above
          (2, (), False, True, 0, True),                          # no source: a profile
          (0, (0,), True, False, CB.CLIP, True),                  # one source, in place, scaled and clipped
          (1, (0, 2), True, True, 0, False),                      # two, dst between
          (3, (3, 3), False, False, 0, True),                     # two, repeated, in place, no multiply
          (0, (1, 2, 3), True, True, CB.CLIP, True),              # three, dst below
          (3, (0, 1, 2, 0), True, False, 0, False),               # four, dst above, repeated
          (2, (0, 1, 2, 3, 3, 2, 1, 0), True, True, 0, True),     # eight, dst among them twice
          (1, (0, 1, 2, 3, 1), False, True, 0, True),             # five, no multiply
          (0, (3, 2, 1, 0, 3, 2), True, False, CB.CLIP, True))    # six, dst among them, clipped
SCRIPT9 = ((8, (0, 1, 2, 3, 4, 5, 6, 7), True, True, 0, True),    # eight distinct sources and a ninth dst, above
           (0, (1, 2, 3, 4, 5, 6, 7, 8), True, False, 0, True),   # ... below
           (4, (8, 7, 6, 5, 4, 3, 2), False, True, CB.CLIP, True))
# pass B, with a run behind each: (dst, src, coef, c0, mode)
RSCRIPT = ((2, (0, 2, 3), True, True, 0), (0, (1, 0), True, False, CB.CLIP))
# periodic: (k, dst, src, coef and c0, mode)
PSCRIPT = ((5, 2, (0, 2), True, 0), (6, 0, (3,), False, 0), (7, 1, (0, 1, 2, 3, 0), True, CB.CLIP), (8, 3, (1, 2, 3), True, 0))

_INPUTS = {}


def inputs(oracle, name):
    """the seven arrays of KINDS[name]: computed once and shared; no test writes them"""
    if name not in _INPUTS:
        shape, ntr, dt, sw = KINDS[name]
        _INPUTS[name] = CB.make_plan_inputs(oracle, shape, ntr, dt, SEED, zeros=not sw.get("norun"))
    return _INPUTS[name]


def new_plan(M, name, variant=None):
    return H.new_plan(M, KINDS[name], name, name in REF, bool(KINDS[name][3].get("tall")), variant)


def model_of(oracle, name, inp=None):
    shape, ntr, dt, _ = KINDS[name]
    m = CB.PlanModelCombine(oracle, *shape, ntr, dt)
    assert m.upload({k: np.array(v, order="F") for k, v in (inp or inputs(oracle, name)).items()}) is None
    return m


def whole(M, p, name, what=("f", "flux")):
    return H.whole(M, p, KINDS[name], what)


def args_of(name, k, nsrc, coef, c0, sl0=0, n=None):
    shape, _, dt, _ = KINDS[name]
    n = shape[0] - sl0 if n is None else n
    return CB.call_args(n, shape[2], nsrc, dt, 500 + k, coef, c0)


def combine(M, p, name, dst, src, coef=None, c0=None, mode=0, sl0=0, n=None, sum=True, call=None):
    """Plan.combine of host coef (n, nzm, nsrc), c0 (n, nzm) -> sum (n, nzm) or None; coef, c0 and the bands are checked.
    call: another callable with Plan.combine's arguments (a shard plan's)."""
    import torch
    shape, _, dt, _ = KINDS[name]
    nx, nz = shape[1], shape[2]
    n = shape[0] - sl0 if n is None else n
    assert coef is None or (coef.shape == (n, nz - 1, len(src)) and coef.dtype == dt)
    assert c0 is None or (c0.shape == (n, nz - 1) and c0.dtype == dt)
    sh = M.combine_shapes(n, nx, nz, len(src))
    ins = {k: nan_banded(a, sh[k]) for k, a in (("coef", coef), ("c0", c0)) if a is not None}
    orig = {k: raw.clone() for k, (raw, _) in ins.items()}
    buf = nan_out(sh["sum"], dt) if sum else None
    view = lambda k: ins[k][1] if k in ins else None
    torch.cuda.synchronize()      # (the plan may run on a stream that does not wait for the one that filled the buffers)
    (call or p.combine)(dst, src, view("coef"), view("c0"), mode, buf[2] if buf else None, sl0, n)
    p.sync()
    torch.cuda.synchronize()
    for k, (raw, _) in ins.items():
        assert torch.equal(raw.view(torch.uint8), orig[k].view(torch.uint8)), f"{k} changed"
    if not buf:
        return None
    raw, pristine, out = buf
    assert H.bands_kept(raw, pristine), "sum: a band byte changed"
    return to_host(out).reshape((n, nz - 1), order="F")


def model_combine(m, dst, src, coef=None, c0=None, mode=0, sl0=0, n=None):
    s = m.combine(dst, src, coef, c0, mode, sl0=sl0, n=n)
    assert not isinstance(s, int), s
    return s


def model_run(m):
    """a run of the model; the -0.0 of the inputs are planted where no run of these scripts returns a -0.0 (the plan kernels
    and the oracle do not agree on the sign of the zero of a cell that held -0.0 and met no flux): asserted here"""
    assert m.run() is None
    f = m.a["f"]
    assert np.isfinite(f).all() and not np.signbit(f[f == 0]).any(), "a run returns -0.0: plant the -0.0 of the inputs elsewhere"


def snap(m):
    return {k: np.array(v, order="F") for k, v in m.export_device().items()}


def same(got, want, what, strict=False):
    for k in ("f", "flux"):
        (assert_bitwise if strict else CB.same)(got[k], want[k], f"{what}: {k}")


def special_inputs(oracle, name):
    """the inputs of pass A -> (inp, the mask of the planted cells)"""
    inp = dict(inputs(oracle, name))
    inp["f"], mask = CB.plant_specials(inp["f"])
    return inp, mask


# ---- 1. every kind of plan: whole plan, every class of the source count, every state
@pytest.mark.parametrize("name", list(KINDS))
def test_every_plan_kind(mpdata, oracle, name):
    M = mpdata
    shape, ntr, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    script = SCRIPT + (SCRIPT9 if ntr == 9 else ())
    inp, mask = special_inputs(oracle, name)
    F0 = inp["f"]
    inner = F0[:, 3:nx + 3]
    assert np.isnan(inner).any() and np.signbit(inner[inner == 0]).any() and (inner == np.inf).any()
    assert (inner == -np.inf).any() or nx == 1
    assert all(mask[..., t].any() for t in range(ntr)) and not mask[:, :3].any() and not mask[:, nx + 3:].any()
    # ---- pass A on the model
    m = model_of(oracle, name, inp)
    want = []
    for k, (dst, src, coef, c0, mode, sm) in enumerate(script):
        a = args_of(name, k, len(src), coef, c0)
        before = np.array(m.a["f"], order="F")
        s = model_combine(m, dst, src, *a, mode)
        new_f, new_s = CB.combine(before, dst, src, *a, bool(mode))
        CB.same(m.a["f"], new_f, "the plan model is the operator")
        CB.same(s, new_s, "the plan model's sum")
        assert_bitwise(new_f[:, :3], before[:, :3], "the halos stay")
        assert_bitwise(new_f[:, nx + 3:], before[:, nx + 3:], "the halos stay")
        for t in range(ntr):
            if t != dst:
                assert_bitwise(new_f[..., t], before[..., t], f"tracer {t} stays")
        if k == 0:
            assert_bitwise(new_f[:, 3:nx + 3, :, dst], before[:, 3:nx + 3, :, src[0]], "the copy")
            assert np.isnan(new_f[:, 3:nx + 3, :, dst]).any()
        assert not np.array_equal(CB.bits(new_f[..., dst]), CB.bits(before[..., dst])), k
        want.append((a, s, snap(m)))
    # ---- pass A on the plan
    p = new_plan(M, name)
    upload(p, inp)
    same(whole(M, p, name), {"f": F0, "flux": inp["flux"]}, f"{name}: the upload", strict=True)
    for k, ((dst, src, coef, c0, mode, sm), (a, ws, w)) in enumerate(zip(script, want)):
        what = f"{name} script {k} (dst {dst}, src {src}, coef {coef}, c0 {c0}, mode {mode})"
        got = combine(M, p, name, dst, src, *a, mode, sum=sm)
        if sm:
            CB.same(got, ws, what + ": sum")
        same(whole(M, p, name), w, what + ": the call", strict=k == 0)
    if sw.get("norun"):
        p.close()
        return
    # ---- pass B: the clean field, a run behind every call
    clean = inputs(oracle, name)
    m = model_of(oracle, name)
    upload(p, clean)
    for k, (dst, src, coef, c0, mode) in enumerate(RSCRIPT):
        what = f"{name} run script {k} (dst {dst}, src {src})"
        a = args_of(name, 20 + k, len(src), coef, c0)
        ws = model_combine(m, dst, src, *a, mode)
        assert_bitwise(combine(M, p, name, dst, src, *a, mode), ws, what + ": sum")
        same(whole(M, p, name), snap(m), what + ": the call", strict=True)
        # a run on the kept velocities = export -> model -> import -> run: seams and the phantom are consistent
        p.run()
        model_run(m)
        same(whole(M, p, name), snap(m), what + ": the call, run", strict=True)
    if name in PERIODIC:
        assert m.set_boundary(PM.PERIODIC) is None
        p.set_boundary(M.BOUNDARY_PERIODIC)
        p.run()
        model_run(m)
        # (5) the halos are stale behind the run; the export hands out wrapped halos of the NEW dst
        # (6) on halos the export just wrapped: those of dst are copies of the OLD field now, the next export wraps again
        # (7) a run right behind the call, no read-back between   (8) back to GIVEN behind a call: the plan holds what an
        # export just before the switch would have returned
        for k, dst, src, opt, mode in PSCRIPT:
            a = args_of(name, k, len(src), opt, opt)
            ws = model_combine(m, dst, src, *a, mode)
            got = combine(M, p, name, dst, src, *a, mode, sum=k != 7)
            if got is not None:
                assert_bitwise(got, ws, f"{name} periodic {k}: sum")
            if k == 7:
                p.run()
                model_run(m)
            if k == 8:
                p.set_boundary(M.BOUNDARY_GIVEN)
                assert m.set_boundary(PM.GIVEN) is None
            e = whole(M, p, name)
            same(e, snap(m), f"{name} periodic {k}", strict=True)
            if k in (5, 6):
                assert_bitwise(e["f"], PM.wrap(np.array(e["f"], order="F")), f"{name} periodic {k}: the halos are wrapped copies of the new interior")
    p.close()
    if name in FAST:
        # FAST: the same bits as EXACT on the uploaded f; after a run against the plan's own export changed by the model
        p = new_plan(M, name, variant=M.VARIANT_FAST)
        upload(p, inp)
        for k in range(3):
            (dst, src, coef, c0, mode, sm), (a, ws, w) = script[k], want[k]
            CB.same(combine(M, p, name, dst, src, *a, mode), ws, f"{name} FAST {k}: sum")
            CB.same(whole(M, p, name, ("f",))["f"], w["f"], f"{name} FAST upload, combine {k}")
        upload(p, clean)
        p.run()
        for k, (dst, src, coef, c0, mode) in enumerate(RSCRIPT):
            E = whole(M, p, name, ("f",))["f"]
            a = args_of(name, 30 + k, len(src), coef, c0)
            got = combine(M, p, name, dst, src, *a, mode)
            want_E, s_E = CB.combine(E, dst, src, *a, bool(mode))
            assert_bitwise(got, s_E, f"{name} FAST run, combine {k}: sum")
            assert_bitwise(whole(M, p, name, ("f",))["f"], want_E, f"{name} FAST run, combine {k}")
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
    "f32-nz28-even": [(1, 3), (5, 1), (2, 2), (1, 4)],
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
# the calls rotate: (dst, src, coef, c0, mode, sum) -- every class of the source count, no source among them: the one form
# that loads nothing but the partner of a split pair
BCALLS = ((2, (), False, True, 0, True), (0, (1, 0, 3), True, True, 0, True), (3, (1,), False, False, 0, False),
          (1, (0, 1, 2, 3, 3), True, False, CB.CLIP, True), (2, (0, 3), False, True, 0, True), (3, (3, 2, 1, 0, 0, 1, 2, 3), True, True, 0, False))


@pytest.mark.parametrize("name", list(BLOCKS))
def test_blocks_leave_the_rest_alone(mpdata, oracle, name):
    """Kinds of SPLIT: the uploaded f of the partner instances holds -0.0 on every second level of column 1
    (CV.plant_negative_zeros) and negative values elsewhere."""
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
        assert all(planted[b].sum() >= ntr * ((nz - 1) // 4) for b in SPLIT[name])
    calls = [(k, sl0, n) + BCALLS[k % len(BCALLS)] for k, (sl0, n) in enumerate(BLOCKS[name])]
    # ---- the model's pass
    m = model_of(oracle, name, inp)
    want = []
    for k, sl0, n, dst, src, coef, c0, mode, sm in calls:
        before = snap(m)
        a = args_of(name, 10 + k, len(src), coef, c0, sl0, n)
        s = model_combine(m, dst, src, *a, mode, sl0, n)
        after = snap(m)
        new = CB.combine(before["f"][sl0:sl0 + n], dst, src, *a, bool(mode))[0]
        assert_bitwise(after["f"][sl0:sl0 + n], new, "inside")
        assert not np.array_equal(after["f"][sl0:sl0 + n], before["f"][sl0:sl0 + n])
        model_run(m)
        want.append((a, s, before, after, snap(m)))
    # ---- the plan's pass
    p = new_plan(M, name)
    upload(p, inp)
    for (k, sl0, n, dst, src, coef, c0, mode, sm), (a, ws, w_before, w_after, w_run) in zip(calls, want):
        what = f"{name} block {sl0, n} dst {dst} src {src} mode {mode}"
        before = whole(M, p, name)
        same(before, w_before, what + ": before", strict=True)
        got = combine(M, p, name, dst, src, *a, mode, sl0, n, sum=sm)
        if sm:
            assert_bitwise(got, ws, what + ": sum")
        after = whole(M, p, name)
        out = np.ones(ncrms, bool)
        out[sl0:sl0 + n] = False
        assert_bitwise(after["f"][out], before["f"][out], what + ": instances outside")
        for t in range(ntr):
            if t != dst:
                assert_bitwise(after["f"][..., t], before["f"][..., t], what + f": tracer {t}")
        assert_bitwise(after["flux"], before["flux"], what + ": flux")
        same(after, w_after, what + ": the call", strict=True)
        if k == 0 and name in SPLIT:
            for b in SPLIT[name]:
                assert out[b] and np.all(np.signbit(after["f"][b][planted[b]]) & (after["f"][b][planted[b]] == 0)), b
                assert all((after["f"][b, 3:nx + 3, :, t] < 0).any() for t in range(ntr)), b
        # a run of every instance (the phantom of an odd plan rides with instance ncrms - 1; a windowed plan refreshes
        # the seams the call marked stale; u, w, rho, rhow, adz enter it) matches the model
        p.run()
        same(whole(M, p, name), w_run, what + ": the call, run", strict=True)
    p.close()


# ---- 3. cross-checks against the calls the plan already has
@pytest.mark.parametrize("name", ["f64-nz28-nx11", "f32-nz28-odd", "f64-nz12-ref", "f64-nz239-tall", "f32-nz72-even"])
def test_cross_checks_against_existing_calls(mpdata, oracle, name):
    """the degenerate form (one source, itself, c0 = d) is Plan.level_add on the interior; sum is Plan.level_stats of dst
    afterwards; a copy has the raw second moment (Plan.level_cov, RAW) of its original"""
    import torch
    M = mpdata
    shape, ntr, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    inp = inputs(oracle, name)
    d = CB.make_c0(ncrms, nz, dt, 61)
    p, q = new_plan(M, name), new_plan(M, name)
    upload(p, inp)
    upload(q, inp)
    s = combine(M, p, name, 1, (1,), None, d)
    q.level_add(to_dev(d), 0, ncrms, AM.ADD, 1)
    q.sync()
    ep, eq = whole(M, p, name), whole(M, q, name)
    assert_bitwise(ep["f"][:, 3:nx + 3], eq["f"][:, 3:nx + 3], f"{name}: combine is level_add on the interior")
    assert not np.array_equal(ep["f"][..., 1], inp["f"][..., 1])
    q.close()
    st = nan_out(M.combine_shapes(ncrms, nx, nz, 1)["sum"], dt)
    p.level_stats(0, ncrms, sum=st[2], first_tracer=1)
    p.sync()
    assert_bitwise(to_host(st[2]), s, f"{name}: sum is level_stats of dst afterwards")
    a = args_of(name, 62, 3, True, True)
    s = combine(M, p, name, 2, (0, 2, 3), *a, CB.CLIP)
    p.level_stats(0, ncrms, sum=st[2], first_tracer=2)
    p.sync()
    assert_bitwise(to_host(st[2]), s, f"{name}: sum is level_stats of dst afterwards, clipped")
    cov = [nan_out(M.level_cov_shapes(ncrms, nx, nz)["cov"], dt) for _ in range(2)]
    p.level_cov(2, 2, cov[0][2], mode=M.LEVEL_COV_RAW)
    combine(M, p, name, 0, (2,), sum=False)
    p.level_cov(0, 0, cov[1][2], mode=M.LEVEL_COV_RAW)
    p.sync()
    torch.cuda.synchronize()
    assert_bitwise(to_host(cov[1][2]), to_host(cov[0][2]), f"{name}: the copy has the second moment of the original")
    assert np.isfinite(to_host(cov[0][2])).all() and to_host(cov[0][2]).any()
    p.close()


# ---- 4. the host form and the array forms
@pytest.mark.parametrize("name", ["f64-nz28-nx11", "f32-nz28-odd", "f64-nz12-ref", "f64-nz72", "f64-nz239-tall"])
def test_host_form(mpdata, oracle, name):
    M = mpdata
    shape, ntr, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    # (sl0, n, dst, src, coef, c0, mode, sum)
    script = ((0, ncrms, 2, (0, 1, 2), True, True, 0, True), (1, ncrms - 1, 0, (), False, True, 0, False),
              (ncrms - 1, 1, 3, (1,), False, False, 0, True), (0, 2, 1, (3, 2, 1, 0, 1), True, False, CB.CLIP, True))
    m = model_of(oracle, name)
    want = []
    for k, (sl0, n, dst, src, coef, c0, mode, sm) in enumerate(script):
        a = args_of(name, 20 + k, len(src), coef, c0, sl0, n)
        s = model_combine(m, dst, src, *a, mode, sl0, n)
        after = snap(m)
        model_run(m)
        want.append((a, s, after, snap(m)))
    p = new_plan(M, name)
    upload(p, inputs(oracle, name))
    for (sl0, n, dst, src, coef, c0, mode, sm), (a, ws, w_call, w_run) in zip(script, want):
        keep = [None if x is None else np.array(x, order="F") for x in a]
        sh = np.full((n, nz - 1), np.nan, dt, order="F") if sm else None
        p.combine_host(dst, list(src), *a, mode, sh, sl0, n)
        for x, kx, nm in zip(a, keep, ("coef", "c0")):
            if x is not None:
                assert_bitwise(x, kx, f"{name} host {sl0, n}: {nm}")
        if sh is not None:
            assert_bitwise(sh, ws, f"{name} host {sl0, n}: sum")
        same(whole(M, p, name), w_call, f"{name} host form {sl0, n}", strict=True)
        p.run()
        same(whole(M, p, name), w_run, f"{name} host form {sl0, n}, run", strict=True)
    with pytest.raises(M.MpdataError):
        p.combine_host(0, (1, 2), a[0][:, :-1], sl0=0, n=2)       # a wrong shape
    p.close()


# 257 and 600 instances: more than one block of 256 threads and a partly filled last one; (2, 1, 70000): the second trip over
# gridDim.y.  f and the coefficients are random, so instance b differs from b - 256 and level k from k - 65535.  Each with a
# block inside the arrays (sl0 > 0).  f carries the planted -0.0, infinities and NaNs.
ARRAYS = {"n257": ((257, 3, 6), 3, (1, 256)), "n600": ((600, 2, 5), 4, (300, 299)), "rows70000": ((2, 1, 70000), 3, (1, 1))}


@pytest.mark.parametrize("case", list(ARRAYS))
@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
def test_array_forms(mpdata, dt, case):
    import torch
    M = mpdata
    (ncrms, nx, nz), ntr, (b0, bn) = ARRAYS[case]
    rng = np.random.default_rng([77, ncrms, ntr])
    f = CB.plant_specials(np.asfortranarray(rng.uniform(-0.5, 0.5, (ncrms, nx + 6, nz - 1, ntr)).astype(dt)))[0]
    calls = (((0, ncrms), ntr - 1, (0, ntr - 1, 1), True, True, 0), ((b0, bn), 0, (ntr - 1,), False, False, 0),
             ((b0, bn), 1, (), False, True, 0), ((0, ncrms), 0, (0, 1, 2, 0, 1, 2, 0, 1), True, True, CB.CLIP))
    for (sl0, n), dst, src, co, c, mode in calls:
        coef, c0 = CB.call_args(n, nz, len(src), dt, 600 + sl0, co, c)
        want, want_s = CB.combine(f[sl0:sl0 + n], dst, src, coef, c0, bool(mode))
        full = np.array(f, order="F")
        full[sl0:sl0 + n] = want
        assert not np.array_equal(CB.bits(full), CB.bits(f))
        if n > 256:
            assert not np.array_equal(want[256:], want[:n - 256]) and not np.array_equal(want_s[256:], want_s[:n - 256])
        if nz - 1 > 65535 and len(src) != 1:
            assert not np.array_equal(want_s[:, 65535:], want_s[:, :nz - 1 - 65535])
        fd = to_dev(f)
        sh = M.combine_shapes(n, nx, nz, len(src))
        ins = {k: nan_banded(a, sh[k]) for k, a in (("coef", coef), ("c0", c0)) if a is not None}
        orig = {k: raw.clone() for k, (raw, _) in ins.items()}
        bd = nan_out(sh["sum"], dt)
        torch.cuda.synchronize()
        M.combine(fd, dst, src, ins["coef"][1] if "coef" in ins else None, ins["c0"][1] if "c0" in ins else None, mode, bd[2], sl0, n)
        torch.cuda.synchronize()
        assert H.bands_kept(bd[0], bd[1])
        for k, (raw, _) in ins.items():
            assert torch.equal(raw.view(torch.uint8), orig[k].view(torch.uint8)), f"{k} changed"
        (assert_bitwise if len(src) == 1 else CB.same)(to_host(fd), full, f"array form {case} block {sl0, n} src {src}: f")
        CB.same(to_host(bd[2]), want_s, f"array form {case} block {sl0, n} src {src}: sum")
        f = full
    # sum skipped
    fd = to_dev(f)
    M.combine(fd, 1, [0, 1])
    torch.cuda.synchronize()
    CB.same(to_host(fd), CB.combine(f, 1, (0, 1))[0], f"array form {case}, two sources alone: f")


# ---- 5. every error code, in the stated order; the plan's state before and after
def test_errors_change_nothing(mpdata, oracle):
    import ctypes
    M = mpdata
    name = "f64-nz28-nx11"
    shape, ntr, dt, _ = KINDS[name]
    ncrms, nx, nz = shape
    inp = inputs(oracle, name)
    c0 = to_dev(CB.make_c0(ncrms, nz, dt, 530))

    def code(fn, *a, **kw):
        with pytest.raises(M.MpdataError) as e:
            fn(*a, **kw)
        return e.value.code

    p = new_plan(M, name)
    assert code(p.combine, 0, (1, 2)) == M.ESTATE                                # never filled
    upload(p, inp)
    before = whole(M, p, name)
    L = M.lib()
    err = L.mpdata_last_error
    ints = lambda *t: ctypes.cast((ctypes.c_int * len(t))(*t), ctypes.c_void_p)
    s12, many = ints(1, 2), ints(*([1] * 9))
    raw = lambda sl0=0, n=ncrms, dst=0, nsrc=2, src=s12, c0=None, mode=0: L.mpdata_plan_combine_device(p._p, sl0, n, dst, nsrc, src, None, c0, mode, None)
    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, ncrms + 1), (ncrms, 1), (3, 3)):
        assert raw(sl0, n) == M.EINVAL, (sl0, n)
    for dst in (-1, ntr):
        assert raw(dst=dst) == M.EINVAL and b"dst" in err(), dst
    for nsrc, src in ((-1, s12), (9, many)):
        assert raw(nsrc=nsrc, src=src) == M.EINVAL and b"nsrc" in err()
    assert raw(src=None) == M.EINVAL and b"null src" in err()
    assert raw(src=ints(1, ntr)) == M.EINVAL and b"src[1]" in err()
    assert raw(src=ints(-1, 0)) == M.EINVAL and b"src[0]" in err()
    assert raw(nsrc=0, src=None) == M.EINVAL and b"null c0" in err()
    for mode in (2, 3, 4, -2):
        assert raw(mode=mode) == M.EINVAL and b"mode" in err(), mode
    # the order: the range, dst, nsrc, src, the sources, c0, the mode
    assert raw(0, 0, 9, 9, None, None, 2) == M.EINVAL and b"n = 0" in err()
    assert raw(dst=9, nsrc=9, src=None, mode=2) == M.EINVAL and b"dst" in err()
    assert raw(nsrc=9, src=None, mode=2) == M.EINVAL and b"nsrc" in err()
    assert raw(src=None, mode=2) == M.EINVAL and b"null src" in err()
    assert raw(src=ints(1, ntr), mode=2) == M.EINVAL and b"src[1]" in err()
    assert raw(nsrc=0, src=None, mode=2) == M.EINVAL and b"null c0" in err()
    assert raw(nsrc=0, src=None, c0=c0.data_ptr(), mode=2) == M.EINVAL and b"mode" in err()
    # a host form of the other precision; its arguments come first
    h32 = lambda dst=0, nsrc=2, src=s12, mode=0: L.mpdata_plan_combine_f32(p._p, 0, ncrms, dst, nsrc, src, None, None, mode, None)
    assert h32() == M.ESTATE
    assert h32(src=None) == M.EINVAL and b"null src" in err()
    assert h32(dst=ntr) == M.EINVAL and h32(mode=2) == M.EINVAL and h32(nsrc=0, src=None) == M.EINVAL
    # the array forms: sizes, the block, f, then dst, the sources and the mode
    one = 8
    arr = lambda ncrms=4, nz=6, sl0=0, n=4, f=one, dst=0, nsrc=2, src=s12, mode=0: \
        L.mpdata_combine_device(ncrms, 5, nz, 3, sl0, n, f, dst, nsrc, src, None, None, mode, None, None)
    assert arr(nz=1, sl0=2, n=3, f=None, dst=9) == M.EINVAL and b"nz=1" in err()
    assert arr(sl0=2, n=3, f=None, dst=9) == M.EINVAL and b"outside" in err()
    assert arr(f=None, dst=9, src=None) == M.EINVAL and b"null f" in err()
    assert arr(dst=3, src=None) == M.EINVAL and b"dst" in err()
    assert arr(src=None, mode=2) == M.EINVAL and b"null src" in err()
    assert arr(src=ints(1, 3), mode=2) == M.EINVAL and b"src[1]" in err()
    assert arr(mode=2) == M.EINVAL and b"mode" in err()
    after = whole(M, p, name)
    for k in before:
        assert_bitwise(after[k], before[k], f"after the refused calls: {k}")
    p.combine(0, (1, 2))                                                         # ... and the plan still works
    p.sync()
    assert not np.array_equal(whole(M, p, name, ("f",))["f"], before["f"])
    p.close()


# ---- 6. a multi-GPU handle is refused; the single-device plans of its shards take the call
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
    c0 = CB.make_c0(ncrms, nz, dt, 540)
    with pytest.raises(M.MpdataError) as e:
        p.combine(0, (1, 2), None, to_dev(c0))
    assert e.value.code == M.EUNSUPPORTED and b"mpdata_plan_shard_plan" in M.lib().mpdata_last_error()
    with pytest.raises(M.MpdataError) as e:
        p.combine_host(0, (1, 2), None, c0)
    assert e.value.code == M.EUNSUPPORTED
    with pytest.raises(M.MpdataError) as e:
        p.combine(9, (9,))                                   # (the handle comes before dst)
    assert e.value.code == M.EUNSUPPORTED
    same(whole(M, p, name), m.export_device(), "after the refused handle calls", strict=True)
    for g, (_, s0, nloc) in enumerate(p.shards()):
        q = p.shard_plan(g)
        dst, src, coef, c, mode, _ = BCALLS[g + 1]
        a = args_of(name, 41 + g, len(src), coef, c, s0, nloc)
        want = model_combine(m, dst, src, *a, mode, s0, nloc)
        got = combine(M, q, name, dst, src, *a, mode, 0, nloc, call=q.combine)
        assert_bitwise(got, want, f"shard {g}: sum")
        q.close()
    same(whole(M, p, name), m.export_device(), "after the shard plans' calls", strict=True)
    p.run()
    model_run(m)
    same(whole(M, p, name), m.export_device(), "after the shard plans' calls and a run", strict=True)
    p.close()


# ---- 7. the Fortran program: every record of its dump against the model
# dtype, program, shape, block, (a source, dst)
FORTRAN = {
    "f64": (F64, "combine_calls", (7, 5, 10), (2, 3), (0, 2)), "f32": (F32, "combine_calls_sp", (6, 5, 10), (1, 3), (2, 0)),
    "f64-whole": (F64, "combine_calls", (5, 3, 28), (0, 5), (1, 0)), "f32-odd-ref": (F32, "combine_calls_sp", (7, 3, 12), (6, 1), (0, 2)),
    "f64-nz72": (F64, "combine_calls", (3, 2, 72), (1, 2), (2, 0)), "f32-nz72": (F32, "combine_calls_sp", (4, 2, 72), (1, 2), (0, 1)),
}


@pytest.mark.parametrize("case", list(FORTRAN))
def test_fortran_program_matches_the_model(oracle, tmp_path, case):
    """the program's calls: dst = coef1 * f(t1) + coef2 * f(dst) + c0 on the block, with sum; t1 = max(dst, 0) on the whole
    plan, with sum; the host form: dst set to a profile on the block; a call with nine sources, refused"""
    dt, exe, shape, (sl0, n), (t1, dst) = FORTRAN[case]
    ncrms, nx, nz = shape
    ntr = 3
    inp = CB.make_plan_inputs(oracle, shape, ntr, dt, SEED + 3, zeros=False)
    coef_a, c0_a = CB.make_coef(n, nz, 2, dt, 700), CB.make_c0(n, nz, dt, 700)
    c0_c = np.asfortranarray(np.abs(CB.make_c0(n, nz, dt, 701)))          # (a run follows: a non-negative profile)
    records = [("params", np.array([ncrms, nx, nz, ntr, sl0, n, t1, dst], np.int64))]
    records += [(k, inp[k]) for k in PM.NAMES] + [("coef_a", coef_a), ("c0_a", c0_a), ("c0_c", c0_c)]
    # the replay on the model
    m = CB.PlanModelCombine(oracle, ncrms, nx, nz, ntr, dt)
    want = FR.want_import(m, inp)
    rc = lambda what, code=None: want.append(FR.rc(what, code))
    sum_a = model_combine(m, dst, (t1, dst), coef_a, c0_a, 0, sl0, n)
    rc("combine_block"); rc("sync")
    want += [("sum_a", sum_a)]
    sum_b = model_combine(m, t1, (dst,), None, None, CB.CLIP)
    rc("combine_clip"); rc("sync")
    want += [("sum_b", sum_b)]
    sum_c = model_combine(m, dst, (), None, c0_c, 0, sl0, n)
    rc("combine_set")
    want += [("sum_c", sum_c)]
    rc("combine_many", m.combine(dst, (t1,) * 9))
    want += FR.want_close(m)
    assert not np.signbit(m.a["f"][m.a["f"] == 0]).any(), "the run returns -0.0 (model_run)"
    FR.compare_dump(FR.run_program(exe, records, tmp_path), want, case)
