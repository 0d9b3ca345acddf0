"""GPU tests of the per-level conditional counts and sums of a resident plan's tracers (include/mpdata_hip.h 3v):
mpdata_plan_level_cond_device, the host forms, the array forms, their Python face Plan.level_cond / level_cond_host /
level_cond, and the Fortran program tests/fortran/level_cond_calls.F90.

Every comparison is bit for bit (util.assert_bitwise) against the numpy model of tests/level_cond_model.py: LC.level_cond
on the field the plan holds -- the plan model's (LC.PlanModelLevelCond: an EXACT plan's f is bit-identical to it) or, for
FAST plans, the plan's own whole export in front of the call.  lo and hi, where given, lie inside larger buffers with 4 KiB
of NaN on both sides, so a read outside the block's arrays poisons the result, and must come back unchanged; cnt and csum
are filled with NaN and lie between two patterned bands of 4 KiB, which must come back unchanged.  Behind every call the
whole export of f and flux must equal the export taken in front of it, and a run behind the calls must equal the model's
run: the call changed nothing, u and w included.

The bounds of a call are drawn from the field the plan holds at that moment (LC.call_args): lo and hi of a row are the
values of two of its own columns, so the ties c == lo (out) and c == hi (in) exist in every row; one level in five is empty
and one in five (three at nx = 3) holds every column.  tests/test_level_cond_cpu.py asserts on the model, for every shape
below, that >= for >, < for <=, a reversed walk, a mask multiplied in and lo of the level below each change at least one
output in ten (fifty): so a passing comparison here tells them apart.

Plans have three tracers; the (tc; first, ntr) triples are (0; 0, 3), (2; 0, 2), (1; 1, 1) and (1; 2, 1) -- tc inside the
range, above it (every value tracer at a negative offset), equal to the only value tracer, and below the only one.  The
outputs are cnt and csum, cnt alone, csum alone; the bounds lo and hi, lo alone, hi alone.

Shapes (ncrms, nx, nz), the smallest at which a path of the kernel differs (NB = 8 columns in flight; the MASK form up to
nx = 64 where two value tracers or more are summed -- the first two triples --, the RE-READ form above and for the others):
  (5, 3, 8)        padding slots of an 8-instance tile, one short batch
  (3, 8, 28)       exactly one batch
  (5, 11, 28), (3, 17, 28)   short last batches
  (3, 3, 64), (3, 2, 65), (3, 9, 72), (2, 2, 140), (2, 2, 238)   63 elements; element 63 | 64 across two slices; three
                   and four slices with idle lanes and an idle wave
  (37, 3, 28), fp32 (74, 3, 28)   19 tiles: more than one thread block of four waves, the last partly filled
  (3, 32, 8), (3, 33, 8)   the mask crosses its first 32-bit word
  (2, 64, 8), (2, 65, 8)   both precisions: the last nx of the MASK form, the first of the RE-READ form
  fp32             pairs (even), the phantom (odd with the switch), the reference layout (odd without it)
  reference layout (5, 3, 12), (6, 3, 12), (7, 3, 12), (2, 3, 250)
  windowed plans   (nz > 238 with set_tall_columns): 239 and 300 levels, 18 instances, fp32 with 15 pseudo-instances (an
                   inner phantom)."""
import itertools

import numpy as np
import pytest

import fortran_records as FR
import level_cond_model as LC
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
    "f64-nz8-nx32": ((3, 32, 8), T, F64, {}), "f64-nz8-nx33": ((3, 33, 8), T, F64, {}),
    "f64-nz8-nx64": ((2, 64, 8), T, F64, {}), "f64-nz8-nx65": ((2, 65, 8), T, F64, {}),
    "f32-nz8-nx64": ((2, 64, 8), T, F32, {}), "f32-nz8-nx65": ((2, 65, 8), T, F32, {}),
    "f32-nz28-even": ((6, 3, 28), T, F32, {}), "f32-nz28-odd": ((7, 3, 28), T, F32, dict(odd=True)),
    "f32-nz72-odd": ((3, 2, 72), T, F32, dict(odd=True)),
    "f64-nz12-ref": ((5, 3, 12), T, F64, dict(ref=True)), "f32-nz12-ref": ((6, 3, 12), T, F32, dict(ref=True)),
    "f32-nz12-odd-ref": ((7, 3, 12), T, F32, {}),      # (an odd fp32 plan without the switch keeps the reference layout)
    "f64-nz250-ref": ((2, 3, 250), T, F64, {}),        # (above 238 levels without the switch: the reference layout)
    "f64-nz239-tall": ((2, 3, 239), T, F64, dict(tall=True)), "f64-nz300-tall": ((3, 2, 300), T, F64, dict(tall=True)),
    "f64-nz239-tall-18": ((18, 2, 239), T, F64, dict(tall=True)),
    "f32-nz239-tall-odd": ((3, 2, 239), T, F32, dict(tall=True, odd=True)),
}
REF = ("f32-nz12-odd-ref", "f64-nz12-ref", "f32-nz12-ref", "f64-nz250-ref")
# one kind of each family runs the FAST variant too; five kinds run a PERIODIC plan
FAST = ("f64-nz28-nx11", "f64-nz72", "f32-nz28-odd", "f64-nz12-ref", "f64-nz239-tall", "f64-nz8-nx65")
PERIODIC = ("f64-nz28-nx11", "f32-nz72-odd", "f64-nz12-ref", "f32-nz239-tall-odd", "f64-nz28-nx17")
TRIPLES = ((0, 0, 3), (2, 0, 2), (1, 1, 1), (1, 2, 1))      # (tc, first, ntr)
OUTS = ("both", "cnt", "csum")
SEED = 100

_INPUTS = {}


def inputs(oracle, name):
    """the seven arrays of KINDS[name]: computed once and shared; no test writes them"""
    if name not in _INPUTS:
        shape, ntr, dt, _ = KINDS[name]
        _INPUTS[name] = LC.make_plan_inputs(oracle, shape, ntr, dt, SEED)
    return _INPUTS[name]


def new_plan(M, name, variant=None):
    return H.new_plan(M, KINDS[name], name, name in REF, bool(KINDS[name][3].get("tall")), variant)


def model_of(oracle, name):
    shape, ntr, dt, _ = KINDS[name]
    m = LC.PlanModelLevelCond(oracle, *shape, ntr, dt)
    assert m.upload({k: np.array(v, order="F") for k, v in inputs(oracle, name).items()}) is None
    return m


def whole(M, p, name, what=("f", "flux")):
    return H.whole(M, p, KINDS[name], what)


def snap(m):
    return {k: np.array(v, order="F") for k, v in m.export_device().items()}


def same(got, want, what):
    for k in ("f", "flux"):
        assert_bitwise(got[k], want[k], f"{what}: {k}")


def level_cond(M, p, name, F, triple, bounds, outs, k, sl0=0, n=None, call=None, given=None):
    """Plan.level_cond on block [sl0, sl0 + n) of the plan whose field is F (ncrms, nx+6, nzm, T), with the bounds of kind
    `bounds` drawn from that block (seed k; given: (lo, hi) to take in their place) and the outputs `outs` -> (lo, hi, cnt,
    csum), the outputs as host arrays (n, nzm) and (n, nzm, ntr) or None.  The bounds and the bands are checked.  call:
    another callable with Plan.level_cond's arguments (a shard plan's)."""
    import torch
    shape, _, dt, _ = KINDS[name]
    nx, nz = shape[1], shape[2]
    n = shape[0] - sl0 if n is None else n
    tc, first, ntr = triple
    lo, hi = given if given is not None else LC.call_args(np.asfortranarray(F[sl0:sl0 + n]), tc, bounds, k)
    sh = M.level_cond_shapes(n, nx, nz, ntr)
    ins = {key: nan_banded(a, sh[key]) for key, a in (("lo", lo), ("hi", hi)) if a is not None}
    orig = {key: r.clone() for key, (r, _) in ins.items()}
    bufs = {key: nan_out(sh[key], dt) for key in ("cnt", "csum") if outs in ("both", key)}
    view = lambda key: ins[key][1] if key in ins else None
    out = lambda key: bufs[key][2] if key in bufs else None
    torch.cuda.synchronize()      # (the plan may run on a stream that does not wait for the one that filled the buffers)
    (call or p.level_cond)(tc, view("lo"), view("hi"), out("cnt"), out("csum"), first, sl0, n)
    p.sync()
    torch.cuda.synchronize()
    for key, (r, _) in ins.items():
        assert torch.equal(r.view(torch.uint8), orig[key].view(torch.uint8)), f"{key} changed"
    res = {}
    for key, (r, pristine, v) in bufs.items():
        assert torch.equal(r[:BAND], pristine[:BAND]) and torch.equal(r[-BAND:], pristine[-BAND:]), f"{key}: a band byte changed"
        res[key] = to_host(v)
    return lo, hi, res.get("cnt"), res.get("csum")


def check(got, F, triple, what, sl0=0, n=None):
    """the outputs of level_cond() against the model on block [sl0, sl0 + n) of the field F"""
    lo, hi, cnt, csum = got
    tc, first, ntr = triple
    n = F.shape[0] - sl0 if n is None else n
    want = LC.level_cond(np.asfortranarray(F[sl0:sl0 + n]), tc, lo, hi, first, ntr)
    assert cnt is not None or csum is not None
    if cnt is not None:
        assert_bitwise(cnt, want[0], what + ": cnt")
    if csum is not None:
        assert_bitwise(csum, want[1], what + ": csum")


# ---- 1. every kind of plan: whole plan, every triple with every set of bounds, the output sets rotating; behind the upload
# and behind a run (a windowed plan's seams and a periodic plan's halos are stale); a run behind the calls
@pytest.mark.parametrize("name", list(KINDS))
def test_every_plan_kind(mpdata, oracle, name):
    M = mpdata
    shape, ntr, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    inp = inputs(oracle, name)
    F0 = inp["f"]
    assert F0.shape == (ncrms, nx + 6, nz - 1, T) and (F0 < 0).any() and (F0 > 0).any()
    m = model_of(oracle, name)
    p = new_plan(M, name)
    upload(p, inp)
    if name in PERIODIC:
        p.set_boundary(M.BOUNDARY_PERIODIC)
        assert m.set_boundary(PM.PERIODIC) is None
    k = 0
    for state in ("upload", "run", "run 2"):
        if state != "upload":
            p.run()
            assert m.run() is None
        before = whole(M, p, name)
        same(before, snap(m), f"{name} {state}: in front of the calls")
        F = m.a["f"]
        combos = list(itertools.product(TRIPLES, LC.BOUNDS))
        if state == "run 2":
            combos = combos[::3]
        for j, (triple, bounds) in enumerate(combos):
            # behind the upload the first and the last triple with every output set; else the sets rotate
            for outs in (OUTS if state == "upload" and triple in (TRIPLES[0], TRIPLES[3]) else (OUTS[(j + j // 3) % 3],)):
                k += 1
                got = level_cond(M, p, name, F, triple, bounds, outs, 300 + k)
                check(got, F, triple, f"{name} {state} triple {triple} bounds {bounds} outputs {outs}")
        same(whole(M, p, name), before, f"{name} {state}: behind the calls")
    p.run()
    assert m.run() is None
    same(whole(M, p, name), snap(m), f"{name}: a run behind the calls")
    p.close()
    if name in FAST:
        # FAST: the same bits as EXACT on the uploaded f; after a run against the plan's own export
        p = new_plan(M, name, variant=M.VARIANT_FAST)
        upload(p, inp)
        for state in ("upload", "run"):
            if state == "run":
                p.run()
            before = whole(M, p, name)
            if state == "upload":
                assert_bitwise(before["f"], F0, f"{name} FAST: the uploaded f")
            for j, (triple, bounds) in enumerate(itertools.product(TRIPLES, LC.BOUNDS)):
                got = level_cond(M, p, name, before["f"], triple, bounds, OUTS[(j + j // 3) % 3], 400 + j)
                check(got, before["f"], triple, f"{name} FAST {state} triple {triple} bounds {bounds}")
            same(whole(M, p, name), before, f"{name} FAST {state}: behind the calls")
        p.close()


# ---- 2. blocks: only the block's instances reach the outputs, and nothing else is written
BLOCKS = {
    # eight instances per tile, five instances: inside the tile, one instance, the last one
    "f64-nz8": [(1, 3), (2, 1), (4, 1), (0, 5)],
    # two per tile: mid-tile to mid-tile, the last (half-filled) tile
    "f64-nz28-nx11": [(1, 3), (4, 1), (0, 4)],
    # 19 tiles in five thread blocks: a block of instances across thread blocks, odd ends, the last instance alone
    "f64-nz28-5blocks": [(7, 11), (3, 32), (36, 1), (8, 8)],
    "f64-nz72": [(1, 1), (1, 2)],
    "f64-nz140": [(1, 1), (0, 1)],
    "f64-nz8-nx33": [(1, 2), (2, 1)],
    "f64-nz8-nx65": [(1, 1), (0, 1)],
    # fp32 pairs: a block that splits pairs at both ends
    "f32-nz28-even": [(1, 3), (5, 1), (2, 2)],
    "f32-nz28-5blocks": [(15, 19), (1, 72), (73, 1)],
    # fp32 pairs, odd plan of 7 (instance 6 shares its pair with the phantom): blocks that hold and miss instance 6, the
    # single-instance block of instance 6 among them
    "f32-nz28-odd": [(1, 2), (6, 1), (5, 2), (0, 6), (3, 3), (0, 7)],
    "f32-nz72-odd": [(2, 1), (1, 1), (0, 2)],
    "f32-nz8-nx64": [(1, 1), (0, 1)],
    "f32-nz12-odd-ref": [(1, 3), (6, 1)],
    "f64-nz12-ref": [(1, 3), (4, 1)],
    # windowed plans: behind an import (the first) and behind a run (the others: stale seams), a block and the whole
    "f64-nz239-tall": [(1, 1), (0, 1), (0, 2)],
    "f64-nz239-tall-18": [(15, 3), (17, 1), (1, 16)],
    "f32-nz239-tall-odd": [(1, 1), (2, 1), (0, 2), (0, 3)],
}


@pytest.mark.parametrize("name", list(BLOCKS))
def test_blocks_reach_only_their_outputs(mpdata, oracle, name):
    """the triples, the bounds and the output sets rotate over the blocks, each block with three calls; a run between the
    blocks"""
    M = mpdata
    m = model_of(oracle, name)
    p = new_plan(M, name)
    upload(p, inputs(oracle, name))
    for b, (sl0, n) in enumerate(BLOCKS[name]):
        if b:
            p.run()
            assert m.run() is None
        before = whole(M, p, name)
        same(before, snap(m), f"{name} block {sl0, n}: in front of the calls")
        for j in range(3):
            triple, bounds, outs = TRIPLES[(b + j) % 4], LC.BOUNDS[(2 * b + j) % 3], OUTS[(b + 2 * j) % 3]
            got = level_cond(M, p, name, m.a["f"], triple, bounds, outs, 500 + 10 * b + j, sl0, n)
            check(got, m.a["f"], triple, f"{name} block {sl0, n} triple {triple} bounds {bounds} outputs {outs}", sl0, n)
        same(whole(M, p, name), before, f"{name} block {sl0, n}: behind the calls")
    p.run()
    assert m.run() is None
    same(whole(M, p, name), snap(m), f"{name}: a run behind the calls")
    p.close()


# ---- 3. selection means selection: +inf and NaN in every EXCLUDED cell of a value tracer never reach csum
@pytest.mark.parametrize("name", ["f64-nz28-nx11", "f32-nz8-nx65"])
def test_plan_excluded_infinities_and_nans_reach_no_sum(mpdata, oracle, name):
    """the planted tracer is imported and never run.  On the model first: a mask multiplied in gives a NaN wherever a
    column is out, the definition gives finite sums"""
    import torch
    M = mpdata
    shape, ntr, dt, sw = KINDS[name]
    F0 = inputs(oracle, name)["f"]
    p = new_plan(M, name)
    upload(p, inputs(oracle, name))
    for tc, t, bounds in ((0, 2, "both"), (2, 1, "lo"), (1, 0, "hi")):
        lo, hi = LC.call_args(F0, tc, bounds, 650 + t)
        P = LC.plant(F0, tc, lo, hi, t)
        assert not np.isfinite(P[..., t]).all() and np.isnan(P[..., t]).any() and np.isposinf(P[..., t]).any()
        want = LC.level_cond(P, tc, lo, hi, 0, T)[1]
        assert np.isfinite(want).all()
        assert np.mean(~np.isfinite(LC.level_cond(P, tc, lo, hi, t, 1, multiply=True)[1])) >= 0.1
        p.import_device(f=to_dev(np.asfortranarray(P[..., t])), first_tracer=t)
        assert_bitwise(whole(M, p, name, ("f",))["f"], P, f"{name}: the planted field")
        for triple in ((tc, 0, T), (tc, t, 1)):
            got = level_cond(M, p, name, P, triple, bounds, "both", 0, given=(lo, hi))
            assert np.isfinite(got[3]).all()
            check(got, P, triple, f"{name} planted tracer {t} under tc {tc} ({bounds}) triple {triple}")
        p.import_device(f=to_dev(np.asfortranarray(F0[..., t])), first_tracer=t)
    p.close()


# ---- 4. the host form and the array forms
@pytest.mark.parametrize("name", ["f64-nz28-nx11", "f32-nz28-odd", "f64-nz12-ref", "f64-nz72", "f64-nz239-tall", "f32-nz8-nx65"])
def test_host_form(mpdata, oracle, name):
    M = mpdata
    shape, ntr, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    # (sl0, n, tc, bounds, outputs): all tracers
    script = ((0, ncrms, 0, "both", "both"), (1, ncrms - 1, 2, "lo", "csum"), (ncrms - 1, 1, 1, "hi", "cnt"), (0, 2, 1, "both", "csum"),
              (0, ncrms, 2, "hi", "both"))
    m = model_of(oracle, name)
    p = new_plan(M, name)
    upload(p, inputs(oracle, name))
    p.run()
    assert m.run() is None
    before = whole(M, p, name)
    for k, (sl0, n, tc, bounds, outs) in enumerate(script):
        lo, hi = LC.call_args(np.asfortranarray(m.a["f"][sl0:sl0 + n]), tc, bounds, 600 + k)
        keep = [None if x is None else np.array(x, order="F") for x in (lo, hi)]
        cnt = np.full((n, nz - 1), np.nan, dt, order="F") if outs != "csum" else None
        csum = np.full((n, nz - 1, T), np.nan, dt, order="F") if outs != "cnt" else None
        p.level_cond_host(tc, lo, hi, cnt, csum, sl0, n)
        for x, kx, nm in zip((lo, hi), keep, ("lo", "hi")):
            if x is not None:
                assert_bitwise(x, kx, f"{name} host {sl0, n}: {nm}")
        check((lo, hi, cnt, csum), m.a["f"], (tc, 0, T), f"{name} host form {sl0, n} tc {tc} {bounds} {outs}", sl0, n)
        same(whole(M, p, name), before, f"{name} host form {sl0, n}")
    with pytest.raises(M.MpdataError):
        p.level_cond_host(0, lo, hi, cnt[:, :-1], None, 0, ncrms)      # a wrong shape
    p.run()
    assert m.run() is None
    same(whole(M, p, name), snap(m), f"{name} host form: a run behind the calls")
    p.close()


# 257 and 600 instances: more than one block of 256 threads and a partly filled last one; (2, 3, 70000): the second trip over
# gridDim.y.  f is random, so instance b differs from b - 256 and level k from k - 65535 (at nx = 2 the counts of the drawn
# bounds would repeat with the levels' period of five, which divides 65535).  Each with a block inside the
# arrays (sl0 > 0).  The last call of every case plants +inf and NaN in the excluded cells of its value tracer.
ARRAYS = {"n257": ((257, 3, 6), 3, (1, 256)), "n600": ((600, 2, 5), 4, (300, 299)), "rows70000": ((2, 3, 70000), 3, (1, 1)),
          "nx65": ((5, 65, 4), 3, (2, 2))}


@pytest.mark.parametrize("case", list(ARRAYS))
@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
def test_array_forms(mpdata, dt, case):
    import torch
    M = mpdata
    (ncrms, nx, nz), ntr_all, (b0, bn) = ARRAYS[case]
    rng = np.random.default_rng([77, ncrms, ntr_all])
    f = np.asfortranarray(rng.uniform(-0.5, 0.5, (ncrms, nx + 6, nz - 1, ntr_all)).astype(dt))
    # ((sl0, n), (tc, first, ntr), bounds, outputs, planted tracer or None)
    calls = (((0, ncrms), (0, 0, ntr_all), "both", "both", None), ((b0, bn), (ntr_all - 1, 0, 2), "lo", "csum", None),
             ((b0, bn), (1, 1, 1), "hi", "both", None), ((0, ncrms), (1, 0, 1), "both", "cnt", None),
             ((b0, bn), (1, 2, 1), "both", "both", 2))
    for k, ((sl0, n), (tc, first, ntr), bounds, outs, planted) in enumerate(calls):
        fb = np.asfortranarray(f[sl0:sl0 + n])
        lo, hi = LC.call_args(fb, tc, bounds, 700 + k)
        g = f
        if planted is not None:
            g = np.array(f, order="F")
            g[sl0:sl0 + n] = LC.plant(fb, tc, lo, hi, planted)
            assert not np.isfinite(g[..., planted]).all()
        fd = to_dev(g)
        want = LC.level_cond(np.asfortranarray(g[sl0:sl0 + n]), tc, lo, hi, first, ntr)
        assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all() and want[0].any() and want[1].any()
        for w in want:
            assert n <= 256 or not np.array_equal(w[256:], w[:n - 256])
            assert nz - 1 <= 65535 or not np.array_equal(w[:, 65535:], w[:, :nz - 1 - 65535])
        sh = M.level_cond_shapes(n, nx, nz, ntr)
        ins = {key: nan_banded(a, sh[key]) for key, a in (("lo", lo), ("hi", hi)) if a is not None}
        orig = {key: r.clone() for key, (r, _) in ins.items()}
        bufs = {key: nan_out(sh[key], dt) for key in ("cnt", "csum") if outs in ("both", key)}
        view = lambda key: ins[key][1] if key in ins else None
        out = lambda key: bufs[key][2] if key in bufs else None
        torch.cuda.synchronize()
        M.level_cond(fd, tc, view("lo"), view("hi"), out("cnt"), out("csum"), first, sl0, n)
        torch.cuda.synchronize()
        for key, (r, _) in ins.items():
            assert torch.equal(r.view(torch.uint8), orig[key].view(torch.uint8)), f"{key} changed"
        for key, w in zip(("cnt", "csum"), want):
            if key in bufs:
                r, pristine, v = bufs[key]
                assert torch.equal(r[:BAND], pristine[:BAND]) and torch.equal(r[-BAND:], pristine[-BAND:]), key
                assert_bitwise(to_host(v), w, f"array form {case} block {sl0, n} triple {tc, first, ntr} {bounds}: {key}")
        assert_bitwise(to_host(fd), g, f"array form {case}: f is only read")


# ---- 5. every error code, in the stated order; the plan's state before and after
def test_errors_change_nothing(mpdata, oracle):
    M = mpdata
    name = "f64-nz28-nx11"
    shape, ntr, dt, _ = KINDS[name]
    ncrms, nx, nz = shape
    inp = inputs(oracle, name)
    import torch
    nan = lambda *sh: torch.full(sh, float("nan"), dtype=torch.float64, device="cuda:0")
    cnt, csum = nan(nz - 1, ncrms), nan(T, nz - 1, ncrms)
    lo_h, hi_h = LC.call_args(inp["f"], 0, "both", 530)
    lo, hi = to_dev(lo_h), to_dev(hi_h)

    def code(fn, *a, **kw):
        with pytest.raises(M.MpdataError) as e:
            fn(*a, **kw)
        return e.value.code

    p = new_plan(M, name)
    assert code(p.level_cond, 0, lo, hi, cnt, csum) == M.ESTATE                  # never filled
    assert code(p.level_cond, 3, lo, hi, cnt, csum) == M.EINVAL                  # ... the arguments come first
    upload(p, inp)
    before = whole(M, p, name)
    L = M.lib()
    err = L.mpdata_last_error
    raw = lambda sl0=0, n=ncrms, tc=0, lo=lo.data_ptr(), hi=hi.data_ptr(), c=cnt.data_ptr(), s=csum.data_ptr(), first=0, ntr=T: \
        L.mpdata_plan_level_cond_device(p._p, sl0, n, tc, lo, hi, c, s, first, ntr)
    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, ncrms + 1), (ncrms, 1), (3, 3)):
        assert raw(sl0, n) == M.EINVAL, (sl0, n)
    for tc in (-1, 3, 9):
        assert raw(tc=tc) == M.EINVAL and b"condition tracer" in err(), tc
    assert raw(lo=None, hi=None) == M.EINVAL and b"lo and hi are both NULL" in err()
    assert raw(c=None, s=None) == M.EINVAL and b"cnt and csum are both NULL" in err()
    for first, n_ in ((0, 0), (-1, 2), (0, 4), (3, 1), (2, 2), (0, -1)):
        assert raw(first=first, ntr=n_) == M.EINVAL and b"tracer range" in err(), (first, n_)
    # the order: the range, tc, the bounds, the outputs, the tracers
    assert raw(0, 0, 9, None, None, None, None, 9, 9) == M.EINVAL and b"n = 0" in err()
    assert raw(tc=9, lo=None, hi=None, c=None, s=None, first=9) == M.EINVAL and b"condition tracer" in err()
    assert raw(lo=None, hi=None, c=None, s=None, first=9) == M.EINVAL and b"lo and hi" in err()
    assert raw(c=None, s=None, first=9) == M.EINVAL and b"cnt and csum" in err()
    assert raw(c=None, first=9) == M.EINVAL and b"tracer range" in err()
    torch.cuda.synchronize()
    assert torch.isnan(cnt).all() and torch.isnan(csum).all()                    # no refused call wrote an output
    # a host form of the other precision; its arguments come first
    c32 = np.full((ncrms, nz - 1), np.nan, F32, order="F")
    l32 = np.zeros((ncrms, nz - 1), F32, order="F")
    h32 = lambda tc=0, lo=l32.ctypes.data, c=c32.ctypes.data: L.mpdata_plan_level_cond_f32(p._p, 0, ncrms, tc, lo, None, c, None)
    assert h32() == M.ESTATE
    assert h32(c=None) == M.EINVAL and b"cnt and csum" in err()
    assert h32(tc=3) == M.EINVAL and h32(lo=None) == M.EINVAL
    assert np.isnan(c32).all()
    # the array forms: sizes, the block, f, then tc, the bounds, the outputs, the tracers
    arr = lambda ncrms=4, nz=6, sl0=0, n=4, f=8, tc=0, lo=8, c=8, s=8, first=0, ntr=3: \
        L.mpdata_level_cond_device(ncrms, 5, nz, 3, sl0, n, f, tc, lo, None, c, s, first, ntr, None)
    assert arr(nz=1, sl0=2, n=3, f=None, tc=3) == M.EINVAL and b"nz=1" in err()
    assert arr(sl0=2, n=3, f=None, tc=3) == M.EINVAL and b"outside" in err()
    assert arr(f=None, tc=3) == M.EINVAL and b"null f" in err()
    assert arr(tc=3, lo=None) == M.EINVAL and b"condition tracer" in err()
    assert arr(lo=None, c=None, s=None) == M.EINVAL and b"lo and hi" in err()
    assert arr(c=None, s=None, ntr=4) == M.EINVAL and b"cnt and csum" in err()
    assert arr(ntr=4) == M.EINVAL and b"tracer range" in err()
    assert arr(first=1, ntr=3) == M.EINVAL and arr(first=-1) == M.EINVAL and arr(ntr=0) == M.EINVAL
    after = whole(M, p, name)
    for k in before:
        assert_bitwise(after[k], before[k], f"after the refused calls: {k}")
    # ... and the plan still works; without csum the tracer range is not looked at
    assert raw(s=None, first=9, ntr=-4) == 0
    p.sync()
    assert_bitwise(to_host(cnt), LC.level_cond(inp["f"], 0, lo_h, hi_h, 0, 0)[0], "the call behind the refused ones")
    assert torch.isnan(csum).all()
    p.close()


# ---- 6. a multi-GPU handle is refused; the single-device plans of its shards take the call
def test_multi_gpu_handle_and_shard_plan(mpdata, oracle, monkeypatch):
    import torch
    M = mpdata
    monkeypatch.delenv("MPDATA_MULTI_XFER", raising=False)
    name = "f64-nz28-nx11"
    shape, ntr, dt, _ = KINDS[name]
    ncrms, nx, nz = shape
    inp = inputs(oracle, name)
    p = M.Plan(*shape, ntr, dtype=dt, devices=[0, 0])
    upload(p, inp)
    m = model_of(oracle, name)
    cnt = torch.full((nz - 1, ncrms), float("nan"), dtype=torch.float64, device="cuda:0")
    lo_h, hi_h = LC.call_args(inp["f"], 0, "both", 540)
    lo = to_dev(lo_h)
    with pytest.raises(M.MpdataError) as e:
        p.level_cond(0, lo, None, cnt)
    assert e.value.code == M.EUNSUPPORTED and b"mpdata_plan_shard_plan" in M.lib().mpdata_last_error()
    with pytest.raises(M.MpdataError) as e:
        p.level_cond_host(0, lo_h, None, np.zeros((ncrms, nz - 1), dt, order="F"))
    assert e.value.code == M.EUNSUPPORTED
    with pytest.raises(M.MpdataError) as e:
        p.level_cond(9, None, None, cnt)                     # (the handle comes before tc and the bounds)
    assert e.value.code == M.EUNSUPPORTED
    torch.cuda.synchronize()
    assert torch.isnan(cnt).all()
    same(whole(M, p, name), m.export_device(), "after the refused handle calls")
    for g, (_, s0, nloc) in enumerate(p.shards()):
        q = p.shard_plan(g)
        for j, bounds in enumerate(LC.BOUNDS):
            triple = TRIPLES[(g + j) % 4]
            Fs = np.asfortranarray(m.a["f"][s0:s0 + nloc])
            got = level_cond(M, q, name, Fs, triple, bounds, OUTS[j], 800 + 10 * g + j, 0, nloc, call=q.level_cond)
            check(got, Fs, triple, f"shard {g} triple {triple} {bounds}")
        q.close()
    same(whole(M, p, name), m.export_device(), "after the shard plans' calls")
    p.run()
    assert m.run() is None
    same(whole(M, p, name), m.export_device(), "after the shard plans' calls and a run")
    p.close()


# ---- 7. the Fortran program: every record of its dump against the model
# dtype, program, shape, block, (t1, tn)
FORTRAN = {
    "f64": (F64, "level_cond_calls", (7, 5, 10), (2, 3), (0, 2)), "f32": (F32, "level_cond_calls_sp", (6, 5, 10), (1, 3), (2, 0)),
    "f64-whole": (F64, "level_cond_calls", (5, 3, 28), (0, 5), (1, 0)), "f32-odd-ref": (F32, "level_cond_calls_sp", (7, 3, 12), (6, 1), (0, 2)),
    "f64-nz72": (F64, "level_cond_calls", (3, 2, 72), (1, 2), (2, 0)), "f32-nz72": (F32, "level_cond_calls_sp", (4, 2, 72), (1, 2), (1, 1)),
    "f64-nx65": (F64, "level_cond_calls", (3, 65, 8), (1, 2), (0, 1)),
}


@pytest.mark.parametrize("case", list(FORTRAN))
def test_fortran_program_matches_the_model(oracle, tmp_path, case):
    """the program's calls: t1 inside (lo_a, hi_a] on the block, cnt and csum of all tracers; tn above lo_b on the whole plan,
    cnt alone with a tracer range that is not looked at; t1 up to hi_c on the whole plan, csum of tracer tn alone; a call
    without a bound, refused"""
    dt, exe, shape, (sl0, n), (t1, tn) = FORTRAN[case]
    ncrms, nx, nz = shape
    inp = LC.make_plan_inputs(oracle, shape, T, dt, SEED + 3)
    lo_a, hi_a = LC.call_args(np.asfortranarray(inp["f"][sl0:sl0 + n]), t1, "both", 900)
    lo_b, _ = LC.call_args(inp["f"], tn, "lo", 901)
    _, hi_c = LC.call_args(inp["f"], t1, "hi", 902)
    records = [("params", np.array([ncrms, nx, nz, T, sl0, n, t1, tn], np.int64))]
    records += [(k, inp[k]) for k in PM.NAMES] + [("lo_a", lo_a), ("hi_a", hi_a), ("lo_b", lo_b), ("hi_c", hi_c)]
    # the replay on the model
    m = LC.PlanModelLevelCond(oracle, ncrms, nx, nz, T, dt)
    want = FR.want_import(m, inp)
    rc = lambda what, code=None: want.append(FR.rc(what, code))
    cnt_a, csum_a = m.level_cond(t1, lo_a, hi_a, 0, T, sl0=sl0, n=n)
    rc("cond_block"); rc("sync")
    want += [("cnt_a", cnt_a), ("csum_a", csum_a)]
    cnt_b, none = m.level_cond(tn, lo_b, None, T, 0, csum=False)
    assert none is None
    rc("cond_lo"); rc("sync")
    want += [("cnt_b", cnt_b)]
    none, csum_c = m.level_cond(t1, None, hi_c, tn, 1, cnt=False)
    assert none is None
    rc("cond_hi"); rc("sync")
    want += [("csum_c", csum_c)]
    rc("cond_refused", m.level_cond(t1, None, None))
    want += FR.want_close(m)
    FR.compare_dump(FR.run_program(exe, records, tmp_path), want, case)
