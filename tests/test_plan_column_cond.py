"""GPU tests of the per-column conditional level counts, tops and paths of a resident plan's tracers (include/mpdata_hip.h
3w): mpdata_plan_column_cond_device, the host forms, the array forms, their Python face Plan.column_cond / column_cond_host
/ column_cond, and the Fortran program tests/fortran/column_cond_calls.F90.

Every comparison is bit for bit (util.assert_bitwise) against the numpy model of tests/column_cond_model.py: CC.column_cond
on the field the plan holds -- the plan model's (CC.PlanModelColumnCond: an EXACT plan's f is bit-identical to it) or, for
FAST plans, the plan's own whole export in front of the call.  lo and hi, where given, lie inside larger buffers with 4 KiB
of NaN on both sides, so a read outside the block's arrays poisons the result, and must come back unchanged; the outputs
are filled with NaN and lie between two patterned bands of 4 KiB, which must come back unchanged.  Behind every call the
whole export of f and flux must equal the export taken in front of it, and a run behind the calls must equal the model's
run: the call changed nothing, u and w included.

The bounds of a call are drawn from the field the plan holds at that moment (CC.call_args, which is
level_cond_model.call_args): lo and hi of a row (b, k) are the values of two of its own columns, so the ties c == lo (out)
and c == hi (in) exist; one level in five is empty and one in five (three at nx = 3) is full.  tests/test_column_cond_cpu.py
asserts on the model, for every shape below, that each variant that is not the definition changes an output.

Plans have three tracers; the (tc; first, ntr) triples are (0; 0, 3), (2; 0, 2), (1; 1, 1) and (1; 2, 1).  The output sets:
all six; kcnt + cover; ktop + kbot; cpath alone; cpath + mass.  The bounds: both, lo alone, hi alone.

Shapes (ncrms, nx, nz), the smallest at which a path of the kernel differs (a workgroup takes UG units and CB columns;
LDS holds CB columns and the rows wgt, lo, hi):
  (5, 3, 8)        8 instances in a tile with padding, UG = 32
  (3, 8, 28), (5, 11, 28), (3, 17, 28)   one batch of columns and several
  (3, 3, 64), (3, 2, 65), (3, 9, 72), (2, 2, 140), (2, 2, 238)   slices; the last two force UG down to where a column
                   fits next to the three rows of the 40 KiB budget: (2, 2, 140) UG = 8 and CB = 1, two batches of one
                   column; (2, 2, 238) UG = 4 and CB = 2, one batch; the in-bits fill two to eight words
  fp32             (6, 3, 28) even; (7, 3, 28) and (3, 2, 72) odd with the switch
  reference layout (5, 3, 12), fp32 (6, 3, 12), fp32 (7, 3, 12) odd without the switch, (2, 3, 250) tall without the switch
  windowed plans   (2, 3, 239) CB = 2: two batches of columns per window at a small nx; (3, 2, 300) one; fp32 (3, 2, 239) odd
  more than one group (column_path_model.GROUP_INPUTS): (40, 7, 28), fp32 (41, 7, 28) odd, (70, 7, 5), (20, 7, 72), (20, 7,
                   250) tall, fp32 (37, 7, 250) tall and odd, with the blocks of group_blocks."""
import itertools

import numpy as np
import pytest

import column_cond_model as CC
import column_path_model as CP
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
    "f32-nz28-even": ((6, 3, 28), T, F32, {}), "f32-nz28-odd": ((7, 3, 28), T, F32, dict(odd=True)),
    "f32-nz72-odd": ((3, 2, 72), T, F32, dict(odd=True)),
    "f64-nz12-ref": ((5, 3, 12), T, F64, dict(ref=True)), "f32-nz12-ref": ((6, 3, 12), T, F32, dict(ref=True)),
    "f32-nz12-odd-ref": ((7, 3, 12), T, F32, {}),      # (an odd fp32 plan without the switch keeps the reference layout)
    "f64-nz250-ref": ((2, 3, 250), T, F64, {}),        # (above 238 levels without the switch: the reference layout)
    "f64-nz239-tall": ((2, 3, 239), T, F64, dict(tall=True)), "f64-nz300-tall": ((3, 2, 300), T, F64, dict(tall=True)),
    "f32-nz239-tall-odd": ((3, 2, 239), T, F32, dict(tall=True, odd=True)),
    # more than one group of units: the shapes of column_path_model.GROUP_INPUTS
    "f64-g40-nz28": ((40, 7, 28), T, F64, {}), "f32-g41-nz28-odd": ((41, 7, 28), T, F32, dict(odd=True)),
    "f64-g70-nz5": ((70, 7, 5), T, F64, {}), "f64-g20-nz72": ((20, 7, 72), T, F64, {}),
    "f64-g20-tall": ((20, 7, 250), T, F64, dict(tall=True)), "f32-g37-tall-odd": ((37, 7, 250), T, F32, dict(tall=True, odd=True)),
}
GROUPS = tuple(k for k in KINDS if "-g" in k)
assert all(KINDS[k][0] == CP.GROUP_INPUTS[k][0] and KINDS[k][2] == CP.GROUP_INPUTS[k][2] for k in GROUPS)
REF = ("f32-nz12-odd-ref", "f64-nz12-ref", "f32-nz12-ref", "f64-nz250-ref")
# one kind of each family runs the FAST variant too; five kinds run a PERIODIC plan
FAST = ("f64-nz28-nx11", "f64-nz72", "f32-nz28-odd", "f64-nz12-ref", "f64-nz239-tall", "f64-g40-nz28")
PERIODIC = ("f64-nz28-nx11", "f32-nz72-odd", "f64-nz12-ref", "f32-nz239-tall-odd", "f64-nz28-nx17")
TRIPLES = ((0, 0, 3), (2, 0, 2), (1, 1, 1), (1, 2, 1))      # (tc, first, ntr)
OUTSETS = (CC.OUTPUTS, ("kcnt", "cover"), ("ktop", "kbot"), ("cpath",), ("cpath", "mass"))
# the seeds of the inputs: 100 where the guard of tests/test_column_cond_cpu.py passes -- a seed that misses a condition is
# replaced here, the conditions stay
SEEDS = dict.fromkeys(KINDS, 100)

_INPUTS = {}


def inputs(oracle, name):
    """the seven arrays of KINDS[name]: computed once and shared; no test writes them"""
    if name not in _INPUTS:
        shape, ntr, dt, _ = KINDS[name]
        _INPUTS[name] = CC.make_plan_inputs(oracle, shape, ntr, dt, SEEDS[name])
    return _INPUTS[name]


def new_plan(M, name, variant=None):
    return H.new_plan(M, KINDS[name], name, name in REF, bool(KINDS[name][3].get("tall")), variant)


def model_of(oracle, name):
    shape, ntr, dt, _ = KINDS[name]
    m = CC.PlanModelColumnCond(oracle, *shape, ntr, dt)
    assert m.upload({k: np.array(v, order="F") for k, v in inputs(oracle, name).items()}) is None
    return m


def whole(M, p, name, what=("f", "flux")):
    return H.whole(M, p, KINDS[name], what)


def snap(m):
    return {k: np.array(v, order="F") for k, v in m.export_device().items()}


def same(got, want, what):
    for k in ("f", "flux"):
        assert_bitwise(got[k], want[k], f"{what}: {k}")


def device_call(M, dt, shapes, lo, hi, outs, call):
    """call(lo, hi, kcnt, kbot, ktop, cpath, cover, mass) with lo, hi between NaN bands and the outputs `outs` NaN-filled
    between patterned bands -> {name: host array}; the bounds and the bands are checked"""
    import torch
    ins = {key: nan_banded(a, shapes[key]) for key, a in (("lo", lo), ("hi", hi)) if a is not None}
    orig = {key: r.clone() for key, (r, _) in ins.items()}
    bufs = {key: nan_out(shapes[key], dt) for key in outs}
    view = lambda key: ins[key][1] if key in ins else None
    torch.cuda.synchronize()      # (the plan may run on a stream that does not wait for the one that filled the buffers)
    call(view("lo"), view("hi"), *[bufs[key][2] if key in bufs else None for key in CC.OUTPUTS])
    torch.cuda.synchronize()
    for key, (r, _) in ins.items():
        assert torch.equal(r.view(torch.uint8), orig[key].view(torch.uint8)), f"{key} changed"
    res = {}
    for key, (r, pristine, v) in bufs.items():
        assert torch.equal(r[:BAND], pristine[:BAND]) and torch.equal(r[-BAND:], pristine[-BAND:]), f"{key}: a band byte changed"
        res[key] = to_host(v)
    return res


def column_cond(M, p, name, F, triple, bounds, outs, k, sl0=0, n=None, given=None):
    """Plan.column_cond on block [sl0, sl0 + n) of plan p whose field is F (ncrms, nx+6, nzm, T), with the bounds of kind
    `bounds` drawn from that block (seed k; given: (lo, hi) to take in their place) -> (lo, hi, {output: host array})"""
    shape, _, dt, _ = KINDS[name]
    n = F.shape[0] - sl0 if n is None else n
    tc, first, ntr = triple
    lo, hi = given if given is not None else CC.call_args(np.asfortranarray(F[sl0:sl0 + n]), tc, bounds, k)
    sh = M.column_cond_shapes(n, shape[1], shape[2], ntr)

    def call(lo_d, hi_d, *o):
        p.column_cond(tc, lo_d, hi_d, *o, first, sl0, n)
        p.sync()
    return lo, hi, device_call(M, dt, sh, lo, hi, outs, call)


def check(got, F, rho, adz, triple, what, sl0=0, n=None):
    """the outputs of column_cond() against the model on block [sl0, sl0 + n) of the arrays"""
    lo, hi, res = got
    tc, first, ntr = triple
    n = F.shape[0] - sl0 if n is None else n
    b = slice(sl0, sl0 + n)
    want = CC.column_cond(np.asfortranarray(F[b]), rho[b], adz[b], tc, lo, hi, first, ntr if "cpath" in res else 0)
    assert res
    for key, v in res.items():
        assert_bitwise(v, want[key], f"{what}: {key}")


# ---- 1. every kind of plan: whole plan, every triple with every set of bounds, the output sets rotating; behind the upload
# and behind a run (a windowed plan's seams and a periodic plan's halos are stale); a run behind the calls
@pytest.mark.parametrize("name", list(KINDS))
def test_every_plan_kind(mpdata, oracle, name):
    M = mpdata
    shape, ntr, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    inp = inputs(oracle, name)
    F0, rho, adz = inp["f"], inp["rho"], inp["adz"]
    assert F0.shape == (ncrms, nx + 6, nz - 1, T)
    m = model_of(oracle, name)
    p = new_plan(M, name)
    upload(p, inp)
    if name in PERIODIC:
        p.set_boundary(M.BOUNDARY_PERIODIC)
        assert m.set_boundary(PM.PERIODIC) is None
    k = 0
    for state in ("upload", "run"):
        if state != "upload":
            p.run()
            assert m.run() is None
        before = whole(M, p, name)
        same(before, snap(m), f"{name} {state}: in front of the calls")
        F = m.a["f"]
        for j, (triple, bounds) in enumerate(itertools.product(TRIPLES, CC.BOUNDS)):
            # behind the upload the first triple with every output set; else the sets rotate
            for outs in (OUTSETS if state == "upload" and j == 0 else (OUTSETS[(j + j // 3 + (state == "run")) % 5],)):
                k += 1
                got = column_cond(M, p, name, F, triple, bounds, outs, 300 + k)
                check(got, F, rho, adz, triple, f"{name} {state} triple {triple} bounds {bounds} outputs {outs}")
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
            for j, (triple, bounds) in enumerate(itertools.product(TRIPLES, CC.BOUNDS)):
                got = column_cond(M, p, name, before["f"], triple, bounds, OUTSETS[(j + j // 3) % 5], 400 + j)
                check(got, before["f"], rho, adz, triple, f"{name} FAST {state} triple {triple} bounds {bounds}")
            same(whole(M, p, name), before, f"{name} FAST {state}: behind the calls")
        p.close()


# ---- 2. blocks: only the block's instances reach the outputs, and nothing else is written
BLOCKS = {
    "f64-nz8": [(1, 3), (2, 1), (4, 1), (0, 5)],
    "f64-nz28-nx11": [(1, 3), (4, 1), (0, 4)],
    "f64-nz72": [(1, 1), (1, 2)],
    "f64-nz238": [(1, 1), (0, 1)],
    "f32-nz28-even": [(1, 3), (5, 1), (2, 2)],
    # fp32 pairs, odd plan of 7 (instance 6 shares its pair with the phantom)
    "f32-nz28-odd": [(1, 2), (6, 1), (5, 2), (0, 6), (3, 3), (0, 7)],
    "f32-nz72-odd": [(2, 1), (1, 1), (0, 2)],
    "f32-nz12-odd-ref": [(1, 3), (6, 1)],
    "f64-nz12-ref": [(1, 3), (4, 1)],
    # windowed plans: behind an import (the first) and behind a run (the others: stale seams)
    "f64-nz239-tall": [(1, 1), (0, 1), (0, 2)],
    "f64-nz300-tall": [(1, 2), (2, 1)],
    "f32-nz239-tall-odd": [(1, 1), (2, 1), (0, 2), (0, 3)],
}
BLOCKS.update({name: list(CP.group_blocks(name)) for name in GROUPS})


@pytest.mark.parametrize("name", list(BLOCKS))
def test_blocks_reach_only_their_outputs(mpdata, oracle, name):
    """the triples, the bounds and the output sets rotate over the blocks, each block with three calls; a run between the
    blocks"""
    M = mpdata
    inp = inputs(oracle, name)
    m = model_of(oracle, name)
    p = new_plan(M, name)
    upload(p, inp)
    for b, (sl0, n) in enumerate(BLOCKS[name]):
        if b:
            p.run()
            assert m.run() is None
        before = whole(M, p, name)
        same(before, snap(m), f"{name} block {sl0, n}: in front of the calls")
        for j in range(3):
            triple, bounds, outs = TRIPLES[(b + j) % 4], CC.BOUNDS[(2 * b + j) % 3], OUTSETS[(b + 2 * j) % 5]
            got = column_cond(M, p, name, m.a["f"], triple, bounds, outs, 500 + 10 * b + j, sl0, n)
            check(got, m.a["f"], inp["rho"], inp["adz"], triple,
                  f"{name} block {sl0, n} triple {triple} bounds {bounds} outputs {outs}", sl0, n)
        same(whole(M, p, name), before, f"{name} block {sl0, n}: behind the calls")
    p.run()
    assert m.run() is None
    same(whole(M, p, name), snap(m), f"{name}: a run behind the calls")
    p.close()


# ---- 3. selection means selection: +inf and NaN in every EXCLUDED cell of a value tracer never reach cpath
@pytest.mark.parametrize("name", ["f64-nz28-nx11", "f32-nz72-odd", "f64-nz239-tall", "f64-nz12-ref"])
def test_plan_excluded_infinities_and_nans_reach_no_path(mpdata, oracle, name):
    """the planted tracer is imported and never run"""
    M = mpdata
    inp = inputs(oracle, name)
    F0, rho, adz = inp["f"], inp["rho"], inp["adz"]
    p = new_plan(M, name)
    upload(p, inp)
    for tc, t, bounds in ((0, 2, "both"), (2, 1, "lo"), (1, 0, "hi")):
        lo, hi = CC.call_args(F0, tc, bounds, 650 + t)
        P = CC.plant(F0, tc, lo, hi, t)
        assert not np.isfinite(P[..., t]).all() and np.isnan(P[..., t]).any() and np.isposinf(P[..., t]).any()
        assert np.isfinite(CC.column_cond(P, rho, adz, tc, lo, hi, 0, T)["cpath"]).all()
        p.import_device(f=to_dev(np.asfortranarray(P[..., t])), first_tracer=t)
        assert_bitwise(whole(M, p, name, ("f",))["f"], P, f"{name}: the planted field")
        for triple in ((tc, 0, T), (tc, t, 1)):
            got = column_cond(M, p, name, P, triple, bounds, ("cpath", "mass"), 0, given=(lo, hi))
            assert np.isfinite(got[2]["cpath"]).all() and np.isfinite(got[2]["mass"]).all()
            check(got, P, rho, adz, triple, f"{name} planted tracer {t} under tc {tc} ({bounds}) triple {triple}")
        p.import_device(f=to_dev(np.asfortranarray(F0[..., t])), first_tracer=t)
    p.close()


# ---- 4. the two identities, on the device: with every level in, cpath and mass have the bits of 3k's path and mass; the
# counts of 3v summed over the levels are the counts of 3w summed over the columns
@pytest.mark.parametrize("name", list(KINDS))
def test_identities_with_column_path_and_level_cond(mpdata, oracle, name):
    import torch
    M = mpdata
    shape, ntr, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    inp = inputs(oracle, name)
    p = new_plan(M, name)
    upload(p, inp)
    p.run()
    tdt = H.tdt(dt)
    nan = lambda sh: torch.full(sh, float("nan"), dtype=tdt, device="cuda:0")
    sh = M.column_cond_shapes(ncrms, nx, nz, T)
    psh = M.column_path_shapes(ncrms, nx, T)
    path, mass = nan(psh["path"]), nan(psh["mass"])
    p.column_path(path, mass, 0, ncrms, 0, T)
    cpath, cmass = nan(sh["cpath"]), nan(sh["mass"])
    hi = torch.full(sh["hi"], float("inf"), dtype=tdt, device="cuda:0")
    torch.cuda.synchronize()
    p.column_cond(1, None, hi, None, None, None, cpath, None, cmass)
    p.sync()
    assert_bitwise(to_host(cpath), to_host(path), f"{name}: cpath with every level in against 3k's path")
    assert_bitwise(to_host(cmass), to_host(mass), f"{name}: mass with every level in against 3k's mass")
    F = whole(M, p, name, ("f",))["f"]
    for tc in range(T):
        lo_h, hi_h = CC.call_args(F, tc, "both", 880 + tc)
        lo_d, hi_d = to_dev(lo_h), to_dev(hi_h)
        cnt, kcnt = nan(M.level_cond_shapes(ncrms, nx, nz, 0)["cnt"]), nan(sh["kcnt"])
        torch.cuda.synchronize()
        p.level_cond(tc, lo_d, hi_d, cnt)
        p.column_cond(tc, lo_d, hi_d, kcnt)
        p.sync()
        a, b = to_host(cnt).astype(np.float64).sum(axis=1), to_host(kcnt).astype(np.float64).sum(axis=1)
        assert a.shape == b.shape == (ncrms,) and np.array_equal(a, b) and a.any(), (name, tc, a, b)
    p.close()


# ---- 5. the host form and the array forms
@pytest.mark.parametrize("name", ["f64-nz28-nx11", "f32-nz28-odd", "f64-nz12-ref", "f64-nz72", "f64-nz239-tall"])
def test_host_form(mpdata, oracle, name):
    M = mpdata
    shape, ntr, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    inp = inputs(oracle, name)
    # (sl0, n, tc, bounds, outputs): all tracers
    script = ((0, ncrms, 0, "both", OUTSETS[0]), (1, ncrms - 1, 2, "lo", OUTSETS[4]), (ncrms - 1, 1, 1, "hi", OUTSETS[1]),
              (0, 2, 1, "both", OUTSETS[3]), (0, ncrms, 2, "hi", OUTSETS[2]))
    m = model_of(oracle, name)
    p = new_plan(M, name)
    upload(p, inp)
    p.run()
    assert m.run() is None
    before = whole(M, p, name)
    hsh = lambda n: {"kcnt": (n, nx), "kbot": (n, nx), "ktop": (n, nx), "cpath": (n, nx, T), "cover": (n,), "mass": (n, T)}
    for k, (sl0, n, tc, bounds, outs) in enumerate(script):
        lo, hi = CC.call_args(np.asfortranarray(m.a["f"][sl0:sl0 + n]), tc, bounds, 600 + k)
        keep = [None if x is None else np.array(x, order="F") for x in (lo, hi)]
        o = {key: np.full(hsh(n)[key], np.nan, dt, order="F") for key in outs}
        p.column_cond_host(tc, lo, hi, *[o.get(key) for key in CC.OUTPUTS], sl0, n)
        for x, kx, nm in zip((lo, hi), keep, ("lo", "hi")):
            if x is not None:
                assert_bitwise(x, kx, f"{name} host {sl0, n}: {nm}")
        check((lo, hi, o), m.a["f"], inp["rho"], inp["adz"], (tc, 0, T), f"{name} host form {sl0, n} tc {tc} {bounds} {outs}", sl0, n)
        same(whole(M, p, name), before, f"{name} host form {sl0, n}")
    with pytest.raises(M.MpdataError):
        p.column_cond_host(0, lo, hi, np.zeros((ncrms, nx + 1), dt, order="F"))      # a wrong shape
    p.run()
    assert m.run() is None
    same(whole(M, p, name), snap(m), f"{name} host form: a run behind the calls")
    p.close()


# 257 and 600 instances: more than one block of 256 threads and a partly filled last one, each with a block inside the
# arrays (sl0 > 0).  f is random, so instance b differs from b - 256.  The last call of every case plants +inf and NaN in
# the excluded cells of its value tracer.
ARRAYS = {"n257": ((257, 3, 6), 3, (1, 256)), "n600": ((600, 2, 5), 4, (300, 299))}


@pytest.mark.parametrize("case", list(ARRAYS))
@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
def test_array_forms(mpdata, dt, case):
    M = mpdata
    (ncrms, nx, nz), ntr_all, (b0, bn) = ARRAYS[case]
    rng = np.random.default_rng([77, ncrms, ntr_all])
    f = np.asfortranarray(rng.uniform(-0.5, 0.5, (ncrms, nx + 6, nz - 1, ntr_all)).astype(dt))
    rho = np.asfortranarray(rng.uniform(0.5, 1.5, (ncrms, nz - 1)).astype(dt))
    adz = np.asfortranarray(rng.uniform(0.5, 1.5, (ncrms, nz - 1)).astype(dt))
    rd, ad = to_dev(rho), to_dev(adz)
    # ((sl0, n), (tc, first, ntr), bounds, outputs, planted tracer or None)
    calls = (((0, ncrms), (0, 0, ntr_all), "both", OUTSETS[0], None), ((b0, bn), (ntr_all - 1, 0, 2), "lo", OUTSETS[4], None),
             ((b0, bn), (1, 1, 1), "hi", OUTSETS[0], None), ((0, ncrms), (1, 0, 1), "both", OUTSETS[1], None),
             ((b0, bn), (0, 0, 1), "both", OUTSETS[2], None), ((b0, bn), (1, 2, 1), "both", OUTSETS[4], 2))
    for k, ((sl0, n), (tc, first, ntr), bounds, outs, planted) in enumerate(calls):
        fb = np.asfortranarray(f[sl0:sl0 + n])
        lo, hi = CC.call_args(fb, tc, bounds, 700 + k)
        g = f
        if planted is not None:
            g = np.array(f, order="F")
            g[sl0:sl0 + n] = CC.plant(fb, tc, lo, hi, planted)
            assert not np.isfinite(g[..., planted]).all()
        fd = to_dev(g)
        path = "cpath" in outs
        want = CC.column_cond(np.asfortranarray(g[sl0:sl0 + n]), rho[sl0:sl0 + n], adz[sl0:sl0 + n], tc, lo, hi, first, ntr if path else 0)
        for key in outs:
            assert np.isfinite(want[key]).all() and want[key].any()
            # (instance b is not instance b - 256: asked of the paths, and of the counts and levels where more than a few rows
            # repeat; not of cover, which is nx wherever every column holds a level that is in)
            if n > 256 and (key in ("cpath", "mass") or (key != "cover" and n - 256 >= 16)):
                assert not np.array_equal(want[key][256:], want[key][:n - 256])
        sh = M.column_cond_shapes(n, nx, nz, ntr)
        res = device_call(M, dt, sh, lo, hi, outs, lambda lo_d, hi_d, *o: M.column_cond(fd, rd, ad, tc, lo_d, hi_d, *o, first, sl0, n))
        for key in outs:
            assert_bitwise(res[key], want[key], f"array form {case} block {sl0, n} triple {tc, first, ntr} {bounds}: {key}")
        assert_bitwise(to_host(fd), g, f"array form {case}: f is only read")
    assert_bitwise(to_host(rd), rho, "rho is only read")
    assert_bitwise(to_host(ad), adz, "adz is only read")


# ---- 6. every error code, in the stated order; the plan's state before and after
def test_errors_change_nothing(mpdata, oracle):
    M = mpdata
    name = "f64-nz28-nx11"
    shape, ntr, dt, _ = KINDS[name]
    ncrms, nx, nz = shape
    inp = inputs(oracle, name)
    import torch
    nan = lambda *sh: torch.full(sh, float("nan"), dtype=torch.float64, device="cuda:0")
    o = {"kcnt": nan(nx, ncrms), "kbot": nan(nx, ncrms), "ktop": nan(nx, ncrms), "cpath": nan(T, nx, ncrms), "cover": nan(ncrms),
         "mass": nan(T, ncrms)}
    lo_h, hi_h = CC.call_args(inp["f"], 0, "both", 530)
    lo, hi = to_dev(lo_h), to_dev(hi_h)

    def code(fn, *a, **kw):
        with pytest.raises(M.MpdataError) as e:
            fn(*a, **kw)
        return e.value.code

    p = new_plan(M, name)
    assert code(p.column_cond, 0, lo, hi, o["kcnt"]) == M.ESTATE                 # never filled
    assert code(p.column_cond, 3, lo, hi, o["kcnt"]) == M.EINVAL                 # ... the arguments come first
    upload(p, inp)
    before = whole(M, p, name)
    L = M.lib()
    err = L.mpdata_last_error
    ptr = {k: v.data_ptr() for k, v in o.items()}

    def raw(sl0=0, n=ncrms, tc=0, lo=lo.data_ptr(), hi=hi.data_ptr(), first=0, ntr=T, **out):
        q = dict(ptr, **out)
        return L.mpdata_plan_column_cond_device(p._p, sl0, n, tc, lo, hi, q["kcnt"], q["kbot"], q["ktop"], q["cpath"], q["cover"],
                                                q["mass"], first, ntr)
    none = dict.fromkeys(CC.OUTPUTS)
    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, ncrms + 1), (ncrms, 1), (3, 3)):
        assert raw(sl0, n) == M.EINVAL, (sl0, n)
    for tc in (-1, 3, 9):
        assert raw(tc=tc) == M.EINVAL and b"condition tracer" in err(), tc
    assert raw(lo=None, hi=None) == M.EINVAL and b"lo and hi are both NULL" in err()
    assert raw(**none) == M.EINVAL and b"every output is NULL" in err()
    assert raw(kcnt=None) == M.EINVAL and b"cover without kcnt" in err()
    assert raw(cpath=None) == M.EINVAL and b"mass without cpath" in err()
    for first, n_ in ((0, 0), (-1, 2), (0, 4), (3, 1), (2, 2), (0, -1)):
        assert raw(first=first, ntr=n_) == M.EINVAL and b"tracer range" in err(), (first, n_)
    # the order: the range, tc, the bounds, the outputs, the pairs, the tracers
    assert raw(0, 0, 9, None, None, 9, 9, **none) == M.EINVAL and b"n = 0" in err()
    assert raw(tc=9, lo=None, hi=None, first=9, **none) == M.EINVAL and b"condition tracer" in err()
    assert raw(lo=None, hi=None, first=9, **none) == M.EINVAL and b"lo and hi" in err()
    assert raw(first=9, **none) == M.EINVAL and b"every output" in err()
    assert raw(first=9, kcnt=None, cpath=None) == M.EINVAL and b"cover without kcnt" in err()
    assert raw(first=9, cover=None, cpath=None) == M.EINVAL and b"mass without cpath" in err()
    assert raw(first=9) == M.EINVAL and b"tracer range" in err()
    torch.cuda.synchronize()
    assert all(torch.isnan(v).all() for v in o.values())                          # no refused call wrote an output
    # a host form of the other precision; its arguments come first
    c32 = np.full((ncrms, nx), np.nan, F32, order="F")
    l32 = np.zeros((ncrms, nz - 1), F32, order="F")
    h32 = lambda tc=0, lo=l32.ctypes.data, c=c32.ctypes.data, cov=None: \
        L.mpdata_plan_column_cond_f32(p._p, 0, ncrms, tc, lo, None, c, None, None, None, cov, None)
    assert h32() == M.ESTATE
    assert h32(c=None) == M.EINVAL and b"every output" in err()
    assert h32(c=None, cov=c32.ctypes.data) == M.EINVAL and b"cover without kcnt" in err()
    assert h32(tc=3) == M.EINVAL and h32(lo=None) == M.EINVAL
    assert np.isnan(c32).all()
    # the array forms: sizes, the block, f, rho, adz, then tc, the bounds, the outputs, the tracers
    arr = lambda ncrms=4, nz=6, sl0=0, n=4, f=8, rho=8, adz=8, tc=0, lo=8, c=8, s=8, ms=None, first=0, ntr=3: \
        L.mpdata_column_cond_device(ncrms, 5, nz, 3, sl0, n, f, rho, adz, tc, lo, None, c, None, None, s, None, ms, first, ntr, None)
    assert arr(nz=1, sl0=2, n=3, f=None, tc=3) == M.EINVAL and b"nz=1" in err()
    assert arr(sl0=2, n=3, f=None, tc=3) == M.EINVAL and b"outside" in err()
    assert arr(f=None, tc=3) == M.EINVAL and b"null f" in err()
    assert arr(rho=None, tc=3) == M.EINVAL and b"null rho" in err()
    assert arr(adz=None, tc=3) == M.EINVAL and b"null adz" in err()
    assert arr(tc=3, lo=None) == M.EINVAL and b"condition tracer" in err()
    assert arr(lo=None, c=None, s=None) == M.EINVAL and b"lo and hi" in err()
    assert arr(c=None, s=None, ntr=4) == M.EINVAL and b"every output" in err()
    assert arr(s=None, ms=8, ntr=4) == M.EINVAL and b"mass without cpath" in err()
    assert arr(ntr=4) == M.EINVAL and b"tracer range" in err()
    assert arr(first=1, ntr=3) == M.EINVAL and arr(first=-1) == M.EINVAL and arr(ntr=0) == M.EINVAL
    after = whole(M, p, name)
    for k in before:
        assert_bitwise(after[k], before[k], f"after the refused calls: {k}")
    # ... and the plan still works; without cpath the tracer range is not looked at
    assert raw(first=9, ntr=-4, cpath=None, mass=None) == 0
    p.sync()
    want = CC.column_cond(inp["f"], inp["rho"], inp["adz"], 0, lo_h, hi_h, 0, 0)
    for key in ("kcnt", "kbot", "ktop", "cover"):
        assert_bitwise(to_host(o[key]), want[key], f"the call behind the refused ones: {key}")
    assert torch.isnan(o["cpath"]).all() and torch.isnan(o["mass"]).all()
    p.close()


# ---- 7. a multi-GPU handle is refused; the single-device plans of its shards take the call
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
    kcnt = torch.full((nx, ncrms), float("nan"), dtype=torch.float64, device="cuda:0")
    lo_h, hi_h = CC.call_args(inp["f"], 0, "both", 540)
    lo = to_dev(lo_h)
    with pytest.raises(M.MpdataError) as e:
        p.column_cond(0, lo, None, kcnt)
    assert e.value.code == M.EUNSUPPORTED and b"mpdata_plan_shard_plan" in M.lib().mpdata_last_error()
    with pytest.raises(M.MpdataError) as e:
        p.column_cond_host(0, lo_h, None, np.zeros((ncrms, nx), dt, order="F"))
    assert e.value.code == M.EUNSUPPORTED
    with pytest.raises(M.MpdataError) as e:
        p.column_cond(9, None, None, kcnt)                   # (the handle comes before tc and the bounds)
    assert e.value.code == M.EUNSUPPORTED
    torch.cuda.synchronize()
    assert torch.isnan(kcnt).all()
    same(whole(M, p, name), m.export_device(), "after the refused handle calls")
    for g, (_, s0, nloc) in enumerate(p.shards()):
        q = p.shard_plan(g)
        for j, bounds in enumerate(CC.BOUNDS):
            triple = TRIPLES[(g + j) % 4]
            b = slice(s0, s0 + nloc)
            Fs = np.asfortranarray(m.a["f"][b])
            got = column_cond(M, q, name, Fs, triple, bounds, OUTSETS[(g + 2 * j) % 5], 800 + 10 * g + j, 0, nloc)
            check(got, Fs, inp["rho"][b], inp["adz"][b], triple, f"shard {g} triple {triple} {bounds}")
        q.close()
    same(whole(M, p, name), m.export_device(), "after the shard plans' calls")
    p.run()
    assert m.run() is None
    same(whole(M, p, name), m.export_device(), "after the shard plans' calls and a run")
    p.close()


# ---- 8. the Fortran program: every record of its dump against the model
# dtype, program, shape, block, (t1, tn)
FORTRAN = {
    "f64": (F64, "column_cond_calls", (7, 5, 10), (2, 3), (0, 2)), "f32": (F32, "column_cond_calls_sp", (6, 5, 10), (1, 3), (2, 0)),
    "f64-whole": (F64, "column_cond_calls", (5, 3, 28), (0, 5), (1, 0)), "f32-odd-ref": (F32, "column_cond_calls_sp", (7, 3, 12), (6, 1), (0, 2)),
    "f64-nz72": (F64, "column_cond_calls", (3, 2, 72), (1, 2), (2, 0)), "f32-nz72": (F32, "column_cond_calls_sp", (4, 2, 72), (1, 2), (1, 1)),
}


@pytest.mark.parametrize("case", list(FORTRAN))
def test_fortran_program_matches_the_model(oracle, tmp_path, case):
    """the program's calls: the device form with t1 inside (lo_a, hi_a] on the block, every output of all tracers; the host
    form with tn above lo_b on the whole plan, kcnt and cover; the array form with t1 up to hi_c on the block of the arrays the
    plan was filled from, cpath and mass of tracer tn alone; a call without a bound, refused"""
    dt, exe, shape, (sl0, n), (t1, tn) = FORTRAN[case]
    ncrms, nx, nz = shape
    inp = CC.make_plan_inputs(oracle, shape, T, dt, 103)
    b = slice(sl0, sl0 + n)
    lo_a, hi_a = CC.call_args(np.asfortranarray(inp["f"][b]), t1, "both", 900)
    lo_b, _ = CC.call_args(inp["f"], tn, "lo", 901)
    _, hi_c = CC.call_args(np.asfortranarray(inp["f"][b]), t1, "hi", 902)
    records = [("params", np.array([ncrms, nx, nz, T, sl0, n, t1, tn], np.int64))]
    records += [(k, inp[k]) for k in PM.NAMES] + [("lo_a", lo_a), ("hi_a", hi_a), ("lo_b", lo_b), ("hi_c", hi_c)]
    # the replay on the model
    m = CC.PlanModelColumnCond(oracle, ncrms, nx, nz, T, dt)
    want = FR.want_import(m, inp)
    rc = lambda what, code=None: want.append(FR.rc(what, code))
    a = m.column_cond(t1, lo_a, hi_a, 0, T, sl0=sl0, n=n)
    rc("cond_block"); rc("sync")
    want += [(k + "_a", a[k]) for k in CC.OUTPUTS]
    h = m.column_cond(tn, lo_b, None, 0, T, eb=np.dtype(dt).itemsize, outs=("kcnt", "cover"))
    rc("cond_host")
    want += [("kcnt_b", h["kcnt"]), ("cover_b", h["cover"])]
    c = CC.column_cond(np.asfortranarray(inp["f"][b]), inp["rho"][b], inp["adz"][b], t1, None, hi_c, tn, 1)
    rc("cond_array"); rc("dsync")
    want += [("cpath_c", c["cpath"][..., 0]), ("mass_c", c["mass"][..., 0])]
    rc("cond_refused", m.column_cond(t1, None, None))
    want += FR.want_close(m)
    FR.compare_dump(FR.run_program(exe, records, tmp_path), want, case)
