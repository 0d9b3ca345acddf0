"""GPU tests of the saturation adjustment of a resident plan's tracers (include/mpdata_hip.h 3y):
mpdata_plan_satadj_device, the host forms, the array forms, their Python face Plan.satadj / satadj_host / satadj, and the
Fortran program tests/fortran/satadj_calls.F90.

Every comparison is bit for bit (util.assert_bitwise) against the numpy model of tests/satadj_model.py: SA.satadj on a
reference-layout truth, or the plan model with the new call (SA.PlanModelSatadj: an EXACT plan's f and flux are
bit-identical to it).  pres and gz lie inside larger buffers with 4 KiB of NaN on both sides, so a read outside the block's
arrays poisons the result; ncld and iters are filled with NaN and lie between two patterned bands of 4 KiB, which must
come back unchanged, and so must pres and gz.  The fields of th and tq follow the recipe of SA.fill_fields for the rows of
the call (a T1 tied to the row's pressure, q up to 1.6 qs(T1), every seventh cell negative, cells with q == qs(T1)
exactly); every fifth row has pres == 0.  Before every call the test asserts ON THE MODEL the conditions of
SA.check_conditions for the rows the call touches (the row with two values of `it` needs nx >= 2 and maxit >= 2).  A run mixes levels, and
a T1 that is no longer tied to p need not converge, so behind a run the test imports fresh fields of the recipe before the
next call; on windowed plans a relax of th half way to the centre of its row (which writes owned levels only) in front of
every second call makes the other copies of th stale again -- a copy of a level that is not its owner's then gives other
counts than the owner --, and the run behind every call must see the new tn and tt in every copy of a level.

Plans have five tracers; the orders (th, tq, tn, tt) put the written tracers above, below and around the read ones
(negative offsets), and the fifth tracer must keep every bit.

Shapes (ncrms, nx, nz): wave-major fp64 (5, 4, 28); fp32 with odd ncrms at nz = 72 under the packed switch (3, 3, 72);
windowed (2, 3, 239) fp64 and (3, 3, 239) fp32 odd; PERIODIC (5, 11, 28); the reference layout (fp32, odd ncrms, nz <= 32,
switch off); nx one below, at and one above NC, the columns a lane iterates at a time (read from mpdata_satadj.h); an even
fp32 plan for the block that splits pairs at both ends."""
import os
import re

import numpy as np
import pytest

import fortran_records as FR
import plan_harness as H
import relax_model as RM
import satadj_model as SA
import subside_model as UM
from oracle import plan_model as PM
from plan_harness import BAND, _defaults, nan_banded, nan_out, upload
from util import assert_bitwise, to_dev, to_host

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
T = 5
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "codesign-kernels_amd", "csrc")
with open(os.path.join(CSRC, "mpdata_satadj.h")) as fh:
    NC = int(re.search(r"#define MPDATA_SATADJ_NC (\d+)", fh.read()).group(1))

# name -> (shape, tracers, dtype, switches)
KINDS = {
    "f64-nz28": ((5, 4, 28), T, F64, {}), "f32-nz72-odd": ((3, 3, 72), T, F32, dict(odd=True)),
    "f64-nz239-tall": ((2, 3, 239), T, F64, dict(tall=True)), "f32-nz239-tall-odd": ((3, 3, 239), T, F32, dict(tall=True, odd=True)),
    "f64-nz28-periodic": ((5, 11, 28), T, F64, dict(periodic=True)),
    "f32-nz12-odd-ref": ((5, 3, 12), T, F32, {}),        # (an odd fp32 plan without the switch keeps the reference layout)
    "f64-nx-at": ((4, NC, 28), T, F64, {}), "f64-nx-above": ((4, NC + 1, 28), T, F64, {}),
    "f32-nz28-even": ((6, 3, 28), T, F32, {}),
}
if NC > 1:                                               # (one column at a time: there is no nx below it)
    KINDS["f64-nx-below"] = ((4, NC - 1, 28), T, F64, {})
REF = ("f32-nz12-odd-ref",)
FAST = ("f64-nz28", "f32-nz72-odd", "f64-nz239-tall")
ORDERS = ((0, 1, 3, 4), (2, 3, 0, 1), (1, 3, 4, 0), (4, 2, 1, 3))     # (th, tq, tn, tt)
SEED = 100

_INPUTS = {}


def inputs(oracle, name):
    """the seven arrays of KINDS[name] (f signed, in [-0.5, 0.5), no -0.0): computed once and shared; no test writes them"""
    if name not in _INPUTS:
        shape, ntr, dt, _ = KINDS[name]
        _INPUTS[name] = UM.make_plan_inputs(oracle, shape, ntr, dt, SEED)
    return _INPUTS[name]


class Model(RM.PlanModelRelax, SA.PlanModelSatadj):
    pass


def new_plan(M, name, variant=None):
    p = H.new_plan(M, KINDS[name], name, name in REF, bool(KINDS[name][3].get("tall")), variant)
    return p


def whole(M, p, name, what=("f", "flux")):
    return H.whole(M, p, KINDS[name], what)


def snap(m):
    return {k: np.array(v, order="F") for k, v in m.export_device().items()}


def same(got, want, what):
    for k in ("f", "flux"):
        assert_bitwise(got[k], want[k], f"{what}: {k}")


def model_run(m):
    """a run of the model; the plan kernels and the oracle do not agree on the sign of the zero a run returns for a cell that
    held -0.0 and met no flux, so the fields hold none where a run follows: asserted here, on the model"""
    assert m.run() is None
    f = m.a["f"]
    assert not np.signbit(f[f == 0]).any(), "a run returns -0.0"


def params(M, par):
    return None if par is None else M.SatadjParams(**par)


def fresh(F, name, k, order, ice, gz_on, sl0=0, n=None, stale=False):
    """the field F (ncrms, nx+6, nzm, T) with th and tq of block [sl0, sl0 + n) refilled by the recipe -> (F_new, pres, gz or
    None, planted), other values per k.  stale: the relax of halfway() will move th of the block in front of the call, so
    tq is made for the th the call meets"""
    shape, _, dt, _ = KINDS[name]
    n = shape[0] - sl0 if n is None else n
    pres, gz = SA.make_rows(n, shape[2], dt, 500 + k)
    gz = gz if gz_on else None
    after = None
    if stale:
        c, tg = halfway(pres, gz)

        def after(h):
            pad = np.zeros((h.shape[0], h.shape[1] + 6, h.shape[2]), h.dtype, order="F")
            pad[:, 3:-3] = h
            return np.array(RM.relax(pad, c, tg[..., 0])[0][:, 3:-3])
    F = np.array(F, order="F")
    F[sl0:sl0 + n], planted = SA.fill_fields(F[sl0:sl0 + n], order[0], order[1], pres, gz, SA.PAR, ice, 500 + k, after=after)
    return np.asfortranarray(F), pres, gz, planted


def conditions(F, name, order, tt_on, pres, gz, par, ice, planted, sl0=0, n=None):
    """the conditions of the call, asserted on the model for the rows it touches"""
    n = F.shape[0] - sl0 if n is None else n
    th, tq, tn, tt = order
    info = SA.satadj(F[sl0:sl0 + n], th, tq, tn, tt if tt_on else -1, pres, gz, par, ice, parts=True)[3]
    SA.check_conditions(info, ice, par["maxit"], planted, rows_differ=F.shape[1] - 6 >= 2)


def satadj(M, p, name, order, tt_on, pres, gz, par, mode, sl0=0, n=None, outs=("ncld", "iters"), call=None):
    """Plan.satadj of host pres, gz (n, nzm) -> {ncld, iters: (n, nzm)} of the outputs asked for; pres, gz and the bands are
    checked.  call: another callable with Plan.satadj's arguments (a shard plan's)."""
    import torch
    shape, _, dt, _ = KINDS[name]
    nx, nz = shape[1], shape[2]
    n = shape[0] - sl0 if n is None else n
    sh = M.satadj_shapes(n, nx, nz)
    ins = {k: nan_banded(a, sh[k]) for k, a in (("pres", pres), ("gz", gz)) if a is not None}
    orig = {k: raw.clone() for k, (raw, _) in ins.items()}
    bufs = {k: nan_out(sh[k], dt) for k in outs}
    view = lambda k: ins[k][1] if k in ins else None
    th, tq, tn, tt = order
    torch.cuda.synchronize()      # (the plan may run on a stream that does not wait for the one that filled the buffers)
    (call or p.satadj)(th, tq, tn, view("pres"), params(M, par), tt if tt_on else -1, view("gz"), mode,
                       bufs["ncld"][2] if "ncld" in bufs else None, bufs["iters"][2] if "iters" in bufs else None, sl0, n)
    p.sync()
    torch.cuda.synchronize()
    for k, (raw, _) in ins.items():
        assert torch.equal(raw.view(torch.uint8), orig[k].view(torch.uint8)), f"{k} changed"
    for k, (raw, pristine, _) in bufs.items():
        assert H.bands_kept(raw, pristine), f"{k}: a band byte changed"
    return {k: to_host(v[2]).reshape((n, nz - 1), order="F") for k, v in bufs.items()}


def halfway(pres, gz):
    """(c, target) of a relax of th half way to the centre of its row's recipe (h = T1 + gz): T1 stays tied to p, within 3 of
    the centre, and moves by up to 3.  relax writes owned levels only: on a windowed plan the other copies of th are stale
    behind it, and a copy that is not its owner's gives other counts than the owner"""
    dt = pres.dtype.type
    p = np.where(pres != 0, pres, dt(500)).astype(np.float64)
    tg = 225.0 + 80.0 * (p - 150.0) / 860.0 + (0.0 if gz is None else gz.astype(np.float64))
    return np.asfortranarray(np.full(pres.shape, 0.5, pres.dtype)), np.asfortranarray(tg.astype(pres.dtype)[..., None])


def model_of(oracle, name, F):
    shape, ntr, dt, sw = KINDS[name]
    m = Model(oracle, *shape, ntr, dt)
    inp = {k: np.array(v, order="F") for k, v in inputs(oracle, name).items()}
    inp["f"] = np.array(F, order="F")
    assert m.upload(inp) is None
    if sw.get("periodic"):
        assert m.set_boundary(PM.PERIODIC) is None
    return m


def plan_of(M, oracle, name, F, variant=None):
    p = new_plan(M, name, variant)
    inp = dict(inputs(oracle, name))
    inp["f"] = F
    upload(p, inp)
    if KINDS[name][3].get("periodic"):
        p.set_boundary(M.BOUNDARY_PERIODIC)
    return p


# ---- 1. every kind of plan: whole plan, every option, a run behind every call
# (order, ICE, gz, tt, outputs, maxit, k of the inputs)
SCRIPT = ((ORDERS[0], 1, True, True, ("ncld", "iters"), 10, 0), (ORDERS[1], 0, False, False, ("ncld", "iters"), 2, 1),
          (ORDERS[2], 1, True, True, ("iters",), 1, 2), (ORDERS[3], 0, True, True, ("ncld",), 10, 3),
          (ORDERS[1], 1, False, False, (), 2, 4))


@pytest.mark.parametrize("name", list(KINDS))
def test_every_plan_kind(mpdata, oracle, name):
    M = mpdata
    shape, ntr, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    # ---- the model's pass
    steps = []
    m = None
    for order, ice, gz_on, tt_on, outs, maxit, k in SCRIPT:
        par = SA.par_with(maxit=maxit)
        stale = bool(sw.get("tall")) and k % 2 == 1
        F, pres, gz, planted = fresh(inputs(oracle, name)["f"] if m is None else m.a["f"], name, k, order, ice, gz_on, stale=stale)
        if m is None:
            m = model_of(oracle, name, F)
        else:
            assert m.import_device({"f": F}) is None
        F0 = F
        if stale:
            d = halfway(pres, gz)
            assert not isinstance(m.relax(d[0], d[1], 0, ncrms, order[0], 1), int)
        else:
            d = None
        before = np.array(m.a["f"], order="F")
        conditions(before, name, order, tt_on, pres, gz, par, ice, planted)
        got = m.satadj(order[0], order[1], order[2], order[3] if tt_on else -1, pres, gz, par, ice)
        assert not isinstance(got, int), got
        new_f = SA.satadj(before, order[0], order[1], order[2], order[3] if tt_on else -1, pres, gz, par, ice)[0]
        assert_bitwise(m.a["f"], new_f, "the plan model is the operator")
        assert_bitwise(new_f[:, :3], before[:, :3], "the halos stay")
        assert_bitwise(new_f[:, nx + 3:], before[:, nx + 3:], "the halos stay")
        rest = [t for t in range(T) if t not in ((order[2], order[3]) if tt_on else (order[2],))]
        assert_bitwise(new_f[..., rest], before[..., rest], "every other tracer stays")
        after_call = snap(m)
        model_run(m)
        steps.append((F0, d, pres, gz, par, got, after_call, snap(m)))
    # ---- the plan's pass
    p = None
    for (order, ice, gz_on, tt_on, outs, maxit, k), (F0, d, pres, gz, par, (wn, wi), w_call, w_run) in zip(SCRIPT, steps):
        what = f"{name} script {k} (order {order}, ice {ice}, gz {gz_on}, tt {tt_on}, maxit {maxit})"
        if p is None:
            p = plan_of(M, oracle, name, F0)
        else:
            p.import_device(f=to_dev(F0))
        if d is not None:
            p.relax(to_dev(d[0]), to_dev(d[1]), None, 0, ncrms, order[0], 1)
        got = satadj(M, p, name, order, tt_on, pres, gz, par, ice, outs=outs)
        if "ncld" in got:
            assert_bitwise(got["ncld"], wn, what + ": ncld")
        if "iters" in got:
            assert_bitwise(got["iters"], wi, what + ": iters")
        same(whole(M, p, name), w_call, what + ": the call")
        # a run on the kept velocities: seams, halos and the phantom are consistent, and the run sees the new tn and tt
        p.run()
        same(whole(M, p, name), w_run, what + ": the call, run")
    p.close()
    if name in FAST:
        order, ice, gz_on, tt_on, outs, maxit, k = SCRIPT[0]
        F0, d, pres, gz, par, (wn, wi), w_call, _ = steps[0]
        p = plan_of(M, oracle, name, F0, variant=M.VARIANT_FAST)
        got = satadj(M, p, name, order, tt_on, pres, gz, par, ice)
        assert_bitwise(got["ncld"], wn, f"{name} FAST: ncld")
        assert_bitwise(got["iters"], wi, f"{name} FAST: iters")
        assert_bitwise(whole(M, p, name, ("f",))["f"], w_call["f"], f"{name} FAST: the same bits as EXACT")
        p.close()


# ---- 2. blocks: what lies outside keeps every bit
BLOCKS = {
    "f64-nz28": [(1, 3), (4, 1), (0, 5), (2, 2)],
    # fp32 pairs: odd sl0 and odd n split pairs at both ends
    "f32-nz28-even": [(1, 3), (5, 1), (2, 2), (1, 5)],
    # fp32 pairs, odd plan of 3 (instance 2 shares its pair with the phantom): blocks that hold and miss it
    "f32-nz72-odd": [(1, 1), (2, 1), (0, 2), (1, 2), (0, 3)],
    "f32-nz12-odd-ref": [(1, 3), (4, 1), (0, 5)],
    "f64-nz239-tall": [(1, 1), (0, 1), (0, 2)],
    "f32-nz239-tall-odd": [(1, 1), (2, 1), (0, 2), (0, 3)],
    "f64-nz28-periodic": [(1, 3), (4, 1)],
    "f64-nx-at": [(1, 3), (0, 2), (3, 1)],
}


@pytest.mark.parametrize("name", list(BLOCKS))
def test_blocks_leave_the_rest_alone(mpdata, oracle, name):
    """the orders, the options and maxit rotate; the first call behind the upload, the others behind a run and a block import
    of fresh fields (all tracers of the block), on windowed plans with a relax of th in front of every second call"""
    M = mpdata
    shape, ntr, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    calls = [(k, sl0, n, ORDERS[k % 4], (k + 1) % 2, k % 3 != 1, k % 2 == 0, (10, 2, 1)[k % 3],
              (("ncld", "iters"), ("iters",), ())[k % 3]) for k, (sl0, n) in enumerate(BLOCKS[name])]
    # ---- the model's pass
    m, want = None, []
    for k, sl0, n, order, ice, gz_on, tt_on, maxit, outs in calls:
        par = SA.par_with(maxit=maxit)
        stale = bool(sw.get("tall")) and k % 2 == 1
        F, pres, gz, planted = fresh(inputs(oracle, name)["f"] if m is None else m.a["f"], name, 10 + k, order, ice, gz_on, sl0, n, stale)
        if m is None:
            m = model_of(oracle, name, F)
        else:
            assert m.import_block(sl0, n, {"f": np.asfortranarray(F[sl0:sl0 + n])}) is None
        d = None
        if stale:
            d = halfway(pres, gz)
            assert not isinstance(m.relax(d[0], d[1], sl0, n, order[0], 1), int)
        before = snap(m)
        conditions(before["f"], name, order, tt_on, pres, gz, par, ice, planted, sl0, n)
        got = m.satadj(order[0], order[1], order[2], order[3] if tt_on else -1, pres, gz, par, ice, sl0=sl0, n=n)
        assert not isinstance(got, int), got
        after = snap(m)
        model_run(m)
        want.append((F, d, pres, gz, par, got, before, after, snap(m)))
    # ---- the plan's pass
    p = None
    for (k, sl0, n, order, ice, gz_on, tt_on, maxit, outs), (F, d, pres, gz, par, (wn, wi), w_before, w_after, w_run) in zip(calls, want):
        what = f"{name} block {sl0, n} order {order} ice {ice} maxit {maxit}"
        if p is None:
            p = plan_of(M, oracle, name, F)
        else:
            p.import_block(sl0, f=to_dev(np.asfortranarray(F[sl0:sl0 + n])))
        if d is not None:
            p.relax(to_dev(d[0]), to_dev(d[1]), None, sl0, n, order[0], 1)
        before = whole(M, p, name)
        same(before, w_before, what + ": before")
        got = satadj(M, p, name, order, tt_on, pres, gz, par, ice, sl0, n, outs)
        if "ncld" in got:
            assert_bitwise(got["ncld"], wn, what + ": ncld")
        if "iters" in got:
            assert_bitwise(got["iters"], wi, what + ": iters")
        after = whole(M, p, name)
        out = np.ones(ncrms, bool)
        out[sl0:sl0 + n] = False
        assert_bitwise(after["f"][out], before["f"][out], what + ": instances outside")
        assert_bitwise(after["flux"], before["flux"], what + ": flux")
        same(after, w_after, what + ": the call")
        p.run()
        same(whole(M, p, name), w_run, what + ": the call, run")
    p.close()


# ---- 3. what the call must not read and must not write: halo columns, rows with pres == 0, the partner of a split pair, esi
# and desi without ICE.  NaN and +-1e300 are planted where nothing is read; -0.0 where nothing is written.  No run follows.
@pytest.mark.parametrize("name", ["f64-nz28", "f32-nz28-even", "f32-nz72-odd", "f32-nz12-odd-ref", "f64-nz239-tall", "f32-nz239-tall-odd",
                                  "f64-nx-at", "f64-nx-above"])
def test_poison_where_nothing_is_read_and_negative_zero_where_nothing_is_written(mpdata, oracle, name):
    M = mpdata
    shape, ntr, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    sl0, n = (1, ncrms - 2) if ncrms >= 5 else (1, 1) if dt == F32 else (0, ncrms - 1)     # (fp32: a pair is split)
    big = dt(1e300) if dt == F64 else dt(3e38)
    for k, (order, ice, tt_on) in enumerate(((ORDERS[0], 0, True), (ORDERS[1], 1, True), (ORDERS[2], 0, False))):
        th, tq, tn, tt = order
        F, pres, gz, planted = fresh(inputs(oracle, name)["f"], name, 30 + k, order, ice, True, sl0, n)
        zero = np.broadcast_to((pres == 0)[:, None, :], (n, nx, nz - 1))
        assert zero.any()
        for t, v in ((th, np.nan), (tq, big), (tn, -big), (tt, np.nan)):
            F[:, :3, :, t] = v                                           # halo columns, every instance
            F[:, nx + 3:, :, t] = v
        blk = F[sl0:sl0 + n]
        for t, v in ((th, np.nan), (tq, -big)):
            blk[:, 3:nx + 3, :, t] = np.where(zero, v, blk[:, 3:nx + 3, :, t])      # the rows with pres == 0: not read
        for t in (tn, tt):
            blk[:, 3:nx + 3, :, t] = np.where(zero, -0.0, blk[:, 3:nx + 3, :, t])    # ... and not written
        out = np.ones(ncrms, bool)
        out[sl0:sl0 + n] = False
        F[out, 3, ::2] = -0.0                                            # outside the block (the partner of a split pair)
        F[out, 3 + nx - 1, 1::2] = np.nan
        par = SA.par_with(esi=[np.nan] * 9, desi=[np.nan] * 9, ls=np.nan, tmin=np.nan, tmax=np.nan) if not ice else dict(SA.PAR)
        conditions(F, name, order, tt_on, pres, gz, par, ice, planted, sl0, n)
        m = model_of(oracle, name, F)
        wn, wi = m.satadj(th, tq, tn, tt if tt_on else -1, pres, gz, par, ice, sl0=sl0, n=n)
        assert not wn[pres == 0].any() and not wi[pres == 0].any() and not np.signbit(wn[pres == 0]).any()
        p = plan_of(M, oracle, name, F)
        got = satadj(M, p, name, order, tt_on, pres, gz, par, ice, sl0, n)
        assert_bitwise(got["ncld"], wn, f"{name} {k}: ncld")
        assert_bitwise(got["iters"], wi, f"{name} {k}: iters")
        e = whole(M, p, name)
        p.close()
        assert_bitwise(e["f"], m.a["f"], f"{name} {k}: f")
        assert np.isfinite(e["f"][sl0:sl0 + n, 3:nx + 3, :, tn][~zero]).all()
        for t in (tn, tt):
            v = e["f"][sl0:sl0 + n, 3:nx + 3, :, t][zero]
            assert np.all(np.signbit(v) & (v == 0)), (name, k, t)
        v = e["f"][out, 3, ::2]
        assert np.all(np.signbit(v) & (v == 0)), (name, k)


# ---- 3b. qq = max(q, 0): on a sane curve qs > 0 and a negative q is dry with or without the clamp, so this test alone uses a
# curve that is none: es = -1 everywhere (de = 0), hence qs = -eps / (p + 1) < 0, and q in (qs, 0) on a third of the cells.
# With the clamp such a cell condenses 0 - qs, without it q - qs.  (The conditions of the recipe do not apply to this field.)
@pytest.mark.parametrize("name", ["f64-nz28", "f32-nz72-odd", "f32-nz12-odd-ref"])
def test_negative_q_counts_as_zero(mpdata, oracle, name):
    M = mpdata
    shape, ntr, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    th, tq, tn, tt = ORDERS[0]
    par = SA.par_with(esw=[-1.0] + [0.0] * 8, desw=[0.0] * 9)
    F, pres, gz, _ = fresh(inputs(oracle, name)["f"], name, 60, ORDERS[0], 0, True)
    qs = (-dt(par["eps"])) / (np.where(pres != 0, pres, dt(500)) - dt(-1))
    u = np.random.default_rng(61).uniform(-1.5, 1.5, (ncrms, nx, nz - 1))
    F[:, 3:nx + 3, :, tq] = (u * np.abs(qs[:, None, :])).astype(dt)
    info = SA.satadj(F, th, tq, tn, tt, pres, gz, par, False, parts=True)[3]
    q = F[:, 3:nx + 3, :, tq]
    between = info["on"] & (q < 0) & (q > info["qs1"])
    assert between.mean() >= 0.2 and info["wet"][between].all() and (info["qs1"][info["on"]] < 0).all()
    assert info["watch"].nonfinite == 0 and info["watch"].subnormal == 0
    m = model_of(oracle, name, F)
    wn, wi = m.satadj(th, tq, tn, tt, pres, gz, par, 0)
    qn = m.a["f"][:, 3:nx + 3, :, tn]
    assert np.all(qn[between] != (q - info["qs1"])[between])            # (what an unclamped q would condense)
    p = plan_of(M, oracle, name, F)
    got = satadj(M, p, name, ORDERS[0], True, pres, gz, par, 0)
    assert_bitwise(got["ncld"], wn, f"{name}: ncld")
    assert_bitwise(got["iters"], wi, f"{name}: iters")
    assert_bitwise(whole(M, p, name, ("f",))["f"], m.a["f"], f"{name}: f")
    p.close()


# ---- 4. the host form and the array forms
@pytest.mark.parametrize("name", ["f64-nz28", "f32-nz72-odd", "f32-nz12-odd-ref", "f64-nz239-tall"])
def test_host_form(mpdata, oracle, name):
    M = mpdata
    shape, ntr, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    # (sl0, n, order, ice, gz, tt, outputs)
    script = ((0, ncrms, ORDERS[0], 1, True, True, True), (1, ncrms - 1, ORDERS[1], 0, False, False, False),
              (ncrms - 1, 1, ORDERS[2], 1, True, True, True))
    m, want = None, []
    for k, (sl0, n, order, ice, gz_on, tt_on, outs) in enumerate(script):
        F, pres, gz, planted = fresh(inputs(oracle, name)["f"] if m is None else m.a["f"], name, 20 + k, order, ice, gz_on, sl0, n)
        if m is None:
            m = model_of(oracle, name, F)
        else:
            assert m.import_device({"f": F}) is None
        conditions(F, name, order, tt_on, pres, gz, SA.PAR, ice, planted, sl0, n)
        got = m.satadj(order[0], order[1], order[2], order[3] if tt_on else -1, pres, gz, SA.PAR, ice, sl0=sl0, n=n)
        after = snap(m)
        model_run(m)
        want.append((F, pres, gz, got, after, snap(m)))
    p = None
    for (sl0, n, order, ice, gz_on, tt_on, outs), (F, pres, gz, (wn, wi), w_call, w_run) in zip(script, want):
        if p is None:
            p = plan_of(M, oracle, name, F)
        else:
            p.import_device(f=to_dev(F))
        keep = [None if x is None else np.array(x, order="F") for x in (pres, gz)]
        o = [np.full((n, nz - 1), np.nan, dt, order="F") if outs else None for _ in range(2)]
        p.satadj_host(order[0], order[1], order[2], pres, params(M, SA.PAR), order[3] if tt_on else -1, gz, ice, o[0], o[1], sl0, n)
        for x, kx, nm in zip((pres, gz), keep, ("pres", "gz")):
            if x is not None:
                assert_bitwise(x, kx, f"{name} host {sl0, n}: {nm}")
        if outs:
            assert_bitwise(o[0], wn, f"{name} host {sl0, n}: ncld")
            assert_bitwise(o[1], wi, f"{name} host {sl0, n}: iters")
        same(whole(M, p, name), w_call, f"{name} host form {sl0, n}")
        p.run()
        same(whole(M, p, name), w_run, f"{name} host form {sl0, n}, run")
    with pytest.raises(M.MpdataError):
        p.satadj_host(0, 1, 2, pres[:, :-1], params(M, SA.PAR), sl0=0, n=1)       # a wrong shape
    p.close()


# 257 and 600 instances: more than one block of 256 threads and a partly filled last one; (2, 1, 70000): the second trip over
# gridDim.y.  Each with a block inside the arrays (sl0 > 0).
ARRAYS = {"n257": ((257, 3, 6), 4, (1, 256)), "n600": ((600, 2, 5), 5, (300, 299)), "rows70000": ((2, 1, 70000), 4, (1, 1))}


@pytest.mark.parametrize("case", list(ARRAYS))
@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
def test_array_forms(mpdata, dt, case):
    import torch
    M = mpdata
    (ncrms, nx, nz), ntr, (b0, bn) = ARRAYS[case]
    rng = np.random.default_rng([77, ncrms, ntr])
    f = np.asfortranarray(rng.uniform(-0.5, 0.5, (ncrms, nx + 6, nz - 1, ntr)).astype(dt))
    for k, ((sl0, n), order, ice, gz_on, tt_on) in enumerate((((0, ncrms), (0, 1, ntr - 1, 2), 1, True, True),
                                                              ((b0, bn), (ntr - 1, 2, 0, 1), 0, False, False))):
        th, tq, tn, tt = order
        tt = tt if tt_on else -1
        pres, gz = SA.make_rows(n, nz, dt, 600 + k)
        gz = gz if gz_on else None
        f[sl0:sl0 + n], planted = SA.fill_fields(f[sl0:sl0 + n], th, tq, pres, gz, SA.PAR, ice, 600 + k)
        want, wn, wi, info = SA.satadj(f[sl0:sl0 + n], th, tq, tn, tt, pres, gz, SA.PAR, ice, parts=True)
        SA.check_conditions(info, ice, 10, planted, rows_differ=nx >= 2)
        full = np.array(f, order="F")
        full[sl0:sl0 + n] = want
        if n > 256:
            assert not np.array_equal(want[256:], want[:n - 256]) and not np.array_equal(wn[256:], wn[:n - 256])
        if nz - 1 > 65535:
            assert not np.array_equal(wn[:, 65535:], wn[:, :nz - 1 - 65535])
        fd = to_dev(f)
        sh = M.satadj_shapes(n, nx, nz)
        ins = {k_: nan_banded(a, sh[k_]) for k_, a in (("pres", pres), ("gz", gz)) if a is not None}
        orig = {k_: raw.clone() for k_, (raw, _) in ins.items()}
        bn_, bi_ = nan_out(sh["ncld"], dt), nan_out(sh["iters"], dt)
        torch.cuda.synchronize()
        M.satadj(fd, th, tq, tn, ins["pres"][1], params(M, SA.PAR), tt, ins["gz"][1] if gz_on else None, ice, bn_[2], bi_[2], sl0, n)
        torch.cuda.synchronize()
        assert H.bands_kept(bn_[0], bn_[1]) and H.bands_kept(bi_[0], bi_[1])
        for k_, (raw, _) in ins.items():
            assert torch.equal(raw.view(torch.uint8), orig[k_].view(torch.uint8)), f"{k_} changed"
        assert_bitwise(to_host(fd), full, f"array form {case} block {sl0, n}: f")
        assert_bitwise(to_host(bn_[2]), wn, f"array form {case} block {sl0, n}: ncld")
        assert_bitwise(to_host(bi_[2]), wi, f"array form {case} block {sl0, n}: iters")
        f = full
    # pres alone, the outputs skipped
    fd = to_dev(f)
    pres, _ = SA.make_rows(ncrms, nz, dt, 650)
    f2, _ = SA.fill_fields(f, 0, 1, pres, None, SA.PAR, False, 650)
    fd = to_dev(f2)
    M.satadj(fd, 0, 1, 2, to_dev(pres), params(M, SA.PAR))
    torch.cuda.synchronize()
    assert_bitwise(to_host(fd), SA.satadj(f2, 0, 1, 2, -1, pres)[0], f"array form {case}, pres alone: f")


# ---- 5. every error code, in the stated order; the plan's state before and after
def test_errors_change_nothing(mpdata, oracle):
    import ctypes
    M = mpdata
    name = "f64-nz28"
    shape, ntr, dt, _ = KINDS[name]
    ncrms, nx, nz = shape
    order = ORDERS[0]
    F, pres, gz, _ = fresh(inputs(oracle, name)["f"], name, 40, order, 1, True)
    w = to_dev(pres)
    par = params(M, SA.PAR)

    def code(fn, *a, **kw):
        with pytest.raises(M.MpdataError) as e:
            fn(*a, **kw)
        return e.value.code

    p = new_plan(M, name)
    assert code(p.satadj, 0, 1, 3, w, par) == M.ESTATE                            # never filled
    inp = dict(inputs(oracle, name))
    inp["f"] = F
    upload(p, inp)
    before = whole(M, p, name)
    L = M.lib()
    err = L.mpdata_last_error
    P = lambda **kw: ctypes.byref(params(M, SA.par_with(**kw)))

    def raw(sl0=0, n=ncrms, th=0, tq=1, tn=3, tt=4, pres=w.data_ptr(), par=ctypes.byref(par), mode=0, plan=p._p):
        return L.mpdata_plan_satadj_device(plan, sl0, n, th, tq, tn, tt, pres, None, par, mode, None, None)
    assert raw(plan=None) == M.EINVAL and b"null plan" in err()
    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, ncrms + 1), (ncrms, 1), (3, 3)):
        assert raw(sl0, n) == M.EINVAL, (sl0, n)
    for kw in (dict(th=-1), dict(th=T), dict(tq=-1), dict(tq=T), dict(tn=-1), dict(tn=T)):
        assert raw(**kw) == M.EINVAL and b"outside the" in err(), kw
    for tt in (-2, T):
        assert raw(tt=tt) == M.EINVAL and b"tt =" in err(), tt
    for kw in (dict(tq=0), dict(tn=0), dict(tn=1), dict(tt=0), dict(tt=1), dict(tt=3)):
        assert raw(**kw) == M.EINVAL and b"not distinct" in err(), kw
    assert raw(pres=None) == M.EINVAL and b"null pres" in err()
    assert raw(par=None) == M.EINVAL and b"null par" in err()
    for maxit in (0, -1, 33):
        assert raw(par=P(maxit=maxit)) == M.EINVAL and b"maxit" in err(), maxit
    for tol in (-1.0, np.nan):
        assert raw(par=P(tol=tol)) == M.EINVAL and b"tol" in err(), tol
    for tmin, tmax in ((273.16, 273.16), (280.0, 270.0), (np.nan, 273.16)):
        assert raw(par=P(tmin=tmin, tmax=tmax), mode=1) == M.EINVAL and b"tmax" in err(), (tmin, tmax)
    for mode in (2, 3, 4, -2):
        assert raw(mode=mode) == M.EINVAL and b"mode" in err(), mode
    # the order: the range, th / tq / tn, tt, two equal, pres, par, maxit, tol, the ramp, the mode
    bad = P(maxit=0, tol=-1.0, tmin=5.0, tmax=1.0)
    assert raw(0, 0, 9, 9, 9, 9, None, None, 3) == M.EINVAL and b"n = 0" in err()
    assert raw(th=9, tt=9, tn=1, pres=None, par=None, mode=3) == M.EINVAL and b"outside the" in err()
    assert raw(tt=9, tn=1, pres=None, par=None, mode=3) == M.EINVAL and b"tt =" in err()
    assert raw(tn=1, pres=None, par=None, mode=3) == M.EINVAL and b"not distinct" in err()
    assert raw(pres=None, par=None, mode=3) == M.EINVAL and b"null pres" in err()
    assert raw(par=None, mode=3) == M.EINVAL and b"null par" in err()
    assert raw(par=bad, mode=3) == M.EINVAL and b"maxit" in err()
    assert raw(par=P(tol=-1.0, tmin=5.0, tmax=1.0), mode=3) == M.EINVAL and b"tol" in err()
    assert raw(par=P(tmin=5.0, tmax=1.0), mode=3) == M.EINVAL and b"tmax" in err()
    assert raw(mode=2) == M.EINVAL and b"mode" in err()
    # a host form of the other precision; its arguments come first
    p32 = np.asfortranarray(pres.astype(F32))
    h32 = lambda tn=3, pres=p32.ctypes.data, mode=0: L.mpdata_plan_satadj_f32(p._p, 0, ncrms, 0, 1, tn, 4, pres, None, ctypes.byref(par), mode, None, None)
    assert h32() == M.ESTATE
    assert h32(pres=None) == M.EINVAL and b"null pres" in err()
    assert h32(tn=1) == M.EINVAL and h32(mode=2) == M.EINVAL and h32(tn=T) == M.EINVAL
    # the array forms: sizes, the block, f, then the tracers, pres, par and the mode
    one = 8
    arr = lambda ncrms=4, nz=6, sl0=0, n=4, f=one, th=0, tn=2, pres=one, par=ctypes.byref(par), mode=0: \
        L.mpdata_satadj_device(ncrms, 5, nz, 4, sl0, n, f, th, 1, tn, 3, pres, None, par, mode, None, None, None)
    assert arr(nz=1, sl0=2, n=3, f=None, pres=None) == M.EINVAL and b"nz=1" in err()
    assert arr(sl0=2, n=3, f=None, pres=None) == M.EINVAL and b"outside" in err()
    assert arr(f=None, tn=1, pres=None) == M.EINVAL and b"null f" in err()
    assert arr(th=4, pres=None) == M.EINVAL and b"outside the" in err()
    assert arr(tn=1, pres=None) == M.EINVAL and b"not distinct" in err()
    assert arr(pres=None, par=None) == M.EINVAL and b"null pres" in err()
    assert arr(par=None, mode=2) == M.EINVAL and b"null par" in err()
    assert arr(mode=2) == M.EINVAL and b"mode" in err()
    after = whole(M, p, name)
    for k in before:
        assert_bitwise(after[k], before[k], f"after the refused calls: {k}")
    assert raw(par=P(tmin=280.0, tmax=270.0), mode=0) == 0                        # ... and the plan still works (without ICE
    p.sync()                                                                      # the ramp is not looked at)
    assert not np.array_equal(whole(M, p, name, ("f",))["f"], before["f"])
    p.close()


# ---- 6. a multi-GPU handle is refused; the single-device plans of its shards take the call
def test_multi_gpu_handle_and_shard_plan(mpdata, oracle, monkeypatch):
    M = mpdata
    monkeypatch.delenv("MPDATA_MULTI_XFER", raising=False)
    name = "f64-nz28"
    shape, ntr, dt, _ = KINDS[name]
    ncrms, nx, nz = shape
    order = ORDERS[0]
    F, pres, gz, planted = fresh(inputs(oracle, name)["f"], name, 41, order, 1, True)
    inp = dict(inputs(oracle, name))
    inp["f"] = F
    p = M.Plan(*shape, ntr, dtype=dt, devices=[0, 0])
    upload(p, inp)
    m = model_of(oracle, name, F)
    par = params(M, SA.PAR)
    with pytest.raises(M.MpdataError) as e:
        p.satadj(0, 1, 3, to_dev(pres), par)
    assert e.value.code == M.EUNSUPPORTED and b"mpdata_plan_shard_plan" in M.lib().mpdata_last_error()
    with pytest.raises(M.MpdataError) as e:
        p.satadj_host(0, 1, 3, pres, par)
    assert e.value.code == M.EUNSUPPORTED
    with pytest.raises(M.MpdataError) as e:
        p.satadj(1, 1, 3, to_dev(pres), par)                    # (the handle comes before the tracers)
    assert e.value.code == M.EUNSUPPORTED
    same(whole(M, p, name), m.export_device(), "after the refused handle calls")
    for g, (_, s0, nloc) in enumerate(p.shards()):
        q = p.shard_plan(g)
        pr, gg = np.asfortranarray(pres[s0:s0 + nloc]), np.asfortranarray(gz[s0:s0 + nloc])
        wn, wi = m.satadj(*order, pr, gg, SA.PAR, 1, sl0=s0, n=nloc)
        got = satadj(M, q, name, order, True, pr, gg, SA.PAR, 1, 0, nloc, call=q.satadj)
        assert_bitwise(got["ncld"], wn, f"shard {g}: ncld")
        assert_bitwise(got["iters"], wi, f"shard {g}: iters")
        q.close()
    same(whole(M, p, name), m.export_device(), "after the shard plans' calls")
    p.run()
    model_run(m)
    same(whole(M, p, name), m.export_device(), "after the shard plans' calls and a run")
    p.close()


# ---- 7. the Fortran program: every record of its dump against the model
# dtype, program, shape, block, order
FORTRAN = {
    "f64": (F64, "satadj_calls", (7, 5, 10), (2, 3), ORDERS[0]), "f32": (F32, "satadj_calls_sp", (6, 5, 10), (1, 3), ORDERS[1]),
    "f64-whole": (F64, "satadj_calls", (5, 3, 28), (0, 5), ORDERS[2]), "f32-odd-ref": (F32, "satadj_calls_sp", (7, 3, 28), (4, 3), ORDERS[3]),
    "f64-nz72": (F64, "satadj_calls", (3, 2, 72), (1, 2), ORDERS[1]), "f32-nz72": (F32, "satadj_calls_sp", (4, 2, 72), (1, 2), ORDERS[0]),
}


@pytest.mark.parametrize("case", list(FORTRAN))
def test_fortran_program_matches_the_model(oracle, tmp_path, case):
    """the program's calls: the block with ICE, gz, tt and both outputs; the whole plan without ICE and tt, maxit = 2, with
    both outputs; a call with tn == tq, refused"""
    dt, exe, shape, (sl0, n), order = FORTRAN[case]
    ncrms, nx, nz = shape
    th, tq, tn, tt = order
    inp = dict(UM.make_plan_inputs(oracle, shape, T, dt, SEED + 3))
    # one set of rows and one field for both calls (neither call writes th or tq); the cells with q == qs(T1) are call a's
    pres_b, gz_b = SA.make_rows(ncrms, nz, dt, 701)
    pres_a, gz_a = np.asfortranarray(pres_b[sl0:sl0 + n]), np.asfortranarray(gz_b[sl0:sl0 + n])
    F, planted = SA.fill_fields(inp["f"], th, tq, pres_b, gz_b, SA.PAR, True, 701)
    inp["f"] = F
    par_b = SA.par_with(maxit=2)
    records = [("params", np.array([ncrms, nx, nz, T, sl0, n, th, tn], np.int64))] + [(k, inp[k]) for k in PM.NAMES]
    records += [("tracers", np.array([tq, tt, SA.PAR["maxit"], par_b["maxit"]], np.int64)), ("pres_a", pres_a), ("gz_a", gz_a),
                ("pres_b", pres_b), ("gz_b", gz_b)]
    # the replay on the model
    m = SA.PlanModelSatadj(oracle, ncrms, nx, nz, T, dt)
    want = FR.want_import(m, inp)
    rc = lambda what, code=None: want.append(FR.rc(what, code))
    info = SA.satadj(m.a["f"][sl0:sl0 + n], th, tq, tn, tt, pres_a, gz_a, SA.PAR, True, parts=True)[3]
    SA.check_conditions(info, True, 10, planted[sl0:sl0 + n])
    ncld_a, iters_a = m.satadj(th, tq, tn, tt, pres_a, gz_a, SA.PAR, SA.ICE, sl0=sl0, n=n)
    rc("satadj_block"); rc("sync")
    want += [("ncld_a", ncld_a), ("iters_a", iters_a)]
    info = SA.satadj(m.a["f"], th, tq, tn, -1, pres_b, gz_b, par_b, False, parts=True)[3]
    SA.check_conditions(info, False, 2)
    ncld_b, iters_b = m.satadj(th, tq, tn, -1, pres_b, gz_b, par_b, 0)
    rc("satadj_whole"); rc("sync")
    want += [("ncld_b", ncld_b), ("iters_b", iters_b)]
    rc("satadj_same", m.satadj(th, tq, tq, -1, pres_b, None, par_b, 0))
    want += FR.want_close(m)
    assert not np.signbit(m.a["f"][m.a["f"] == 0]).any(), "the run returns -0.0 (model_run)"
    FR.compare_dump(FR.run_program(exe, records, tmp_path), want, case)
