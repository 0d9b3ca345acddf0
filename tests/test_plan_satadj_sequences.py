"""GPU tests: seeded call orders that interleave import, block import, block export, run, satadj, satadj with ICE, convert
from tn (the cloud water the adjustment made), relax, sediment, export and set_boundary on one resident plan of five
tracers -- wave-major fp64, odd fp32 at nz = 72, a windowed plan, and a plan that is PERIODIC from the start --, side by
side with the plan model that holds sections 3n, 3r, 3t and 3y (tests/sediment_model.py, relax_model.py, convert_model.py,
satadj_model.py).

Every return code is compared; after every satadj the call's ncld and iters must be the model's bit for bit -- they are
functions of every interior value of th and tq the plan holds for the block at that moment --; every export and the final
one must match.  The point is the marks across calls, of the two WRITTEN tracers: a windowed plan meets satadj with fresh
seams (behind an import), with stale ones (behind a run) and with seams a call marked stale (behind another satadj, a
convert, a relax or a sediment), and the call that follows -- a sediment, which refreshes stale seams before it reads a
neighbour level, a run -- must see the NEW tn and tt in every copy of a level; a periodic plan meets it with stale and with
wrapped halos, and the run or read-back that follows must see wrapped copies of the new fields.

A run mixes levels, and a T1 that is no longer tied to the row's pressure need not converge (tests/satadj_model.py), so
the satadj op first imports th and tq of its block afresh by the recipe (a block import of one tracer each: tn and tt keep
the marks the calls before left them with), asserts the conditions of SA.check_conditions on the model, and then calls.  A
drawn block of fewer than MIN_CELLS cells is too small for the shares the conditions ask for: the op then takes the whole
plan, so every satadj of a sequence asserts every condition.

The driver and the plain forms of the other ops: tests/plan_harness.py."""
import numpy as np
import pytest

import convert_model as CV
import plan_harness as H
import relax_model as RM
import satadj_model as SA
import sediment_model as SM
import subside_model as UM
from plan_harness import _defaults
from util import assert_bitwise, to_dev, to_host

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
# name, shape, tracers, dtype, switches, seed
CASES = [("wm-f64-nz28", (5, 4, 28), 5, F64, {}, 91), ("f32-odd-nz72", (3, 3, 72), 5, F32, dict(odd=True), 92),
         ("tall-f64-nz239", (2, 3, 239), 5, F64, dict(tall=True), 93),
         ("periodic-f64-nz28-nx11", (5, 11, 28), 5, F64, dict(periodic=True), 94)]
STEPS = 28
OPS = ("import", "import_block", "export_block", "run", "satadj", "satadj_ice", "convert", "relax", "sediment", "export", "set_boundary",
       "satadj_refused")
ORDERS = ((0, 1, 3, 4), (2, 3, 0, 1), (1, 3, 4, 0), (4, 2, 1, 3))     # (th, tq, tn, tt)
# a satadj op whose drawn block holds fewer cells takes the whole plan: a third of them is saturated, and each of the three
# regimes must hold a tenth of those
MIN_CELLS = 400


class Model(SM.PlanModelSediment, RM.PlanModelRelax, CV.PlanModelConvert, SA.PlanModelSatadj):
    pass


def satadj(s, sl0, n, first, ntr):
    """(both ops, satadj and satadj_ice; no draw; the tracer range of the step is not used: the orders rotate; a block below
    MIN_CELLS cells becomes the whole plan) th and tq of
    the block imported afresh; pres and gz between NaN bands, gz and tt on two calls of three, maxit 10, 2, 1 in turn, ncld and
    iters NaN-filled between patterned bands"""
    import torch
    c = s.count["satadj"] + s.count["satadj_ice"]
    if n * s.nx * (s.nz - 1) < MIN_CELLS:
        sl0, n = 0, s.ncrms
    order = th, tq, tn, tt = ORDERS[c % 4]
    ice = int(s.op == "satadj_ice")
    gz_on, tt_on, maxit = c % 3 != 1, c % 3 != 2, (10, 2, 1)[(c // 2) % 3]
    s.last = order
    par = SA.par_with(maxit=maxit)
    pres, gz = SA.make_rows(n, s.nz, s.dt, s.seed_of_step())
    gz = gz if gz_on else None
    blk, planted = SA.fill_fields(s.m.a["f"][sl0:sl0 + n], th, tq, pres, gz, SA.PAR, bool(ice), s.seed_of_step())
    for t in (th, tq):
        one = np.asfortranarray(blk[..., t])
        assert s.code(s.p.import_block, sl0, f=to_dev(one), first_tracer=t) is None
        assert s.m.import_block(sl0, n, {"f": one}, t, 1) is None
    info = SA.satadj(s.m.a["f"][sl0:sl0 + n], th, tq, tn, tt if tt_on else -1, pres, gz, par, bool(ice), parts=True)[3]
    SA.check_conditions(info, bool(ice), maxit, planted)
    sh = s.M.satadj_shapes(n, s.nx, s.nz)
    ins = {k: H.nan_banded(a, sh[k]) for k, a in (("pres", pres), ("gz", gz)) if a is not None}
    view = lambda k: ins[k][1] if k in ins else None
    bufs = {k: H.nan_out(sh[k], s.dt) for k in ("ncld", "iters")}
    torch.cuda.synchronize()
    assert s.code(s.p.satadj, th, tq, tn, view("pres"), s.M.SatadjParams(**par), tt if tt_on else -1, view("gz"), ice,
                  bufs["ncld"][2], bufs["iters"][2], sl0, n) is None
    s.p.sync()
    want = s.m.satadj(th, tq, tn, tt if tt_on else -1, pres, gz, par, ice, sl0=sl0, n=n)
    for k, w in zip(("ncld", "iters"), want):
        raw, pristine, out = bufs[k]
        assert H.bands_kept(raw, pristine)
        assert_bitwise(to_host(out), w, s.at(f"{k} of order {order}", sl0, n, first, ntr))


def satadj_refused(s, sl0, n, first, ntr):
    M, ncrms, T = s.M, s.ncrms, s.T
    pres, _ = SA.make_rows(1, s.nz, s.dt, s.seed_of_step())
    # (sl0, n, th, tq, tn, tt, mode, par)
    bad = [(ncrms, 1, 0, 1, 2, 3, 0, SA.PAR), (0, 1, T, 1, 2, 3, 0, SA.PAR), (0, 1, 0, 1, 1, 3, 0, SA.PAR), (0, 1, 0, 1, 2, 3, 2, SA.PAR),
           (0, 1, 0, 1, 2, 3, 1, SA.par_with(tmin=300.0)), (0, 1, 0, 1, 2, 3, 0, SA.par_with(maxit=0))][s.count[s.op] % 6]
    got = s.code(s.p.satadj, bad[2], bad[3], bad[4], to_dev(pres), M.SatadjParams(**bad[7]), bad[5], None, bad[6], None, None, bad[0], bad[1])
    assert got == M.EINVAL == s.m.satadj(bad[2], bad[3], bad[4], bad[5], pres, None, bad[7], bad[6], sl0=bad[0], n=bad[1])


def convert(s, sl0, n, first, ntr):
    """convert from tn, the condensate of the last satadj, to the tracer below it (autoconversion), r alone"""
    src = getattr(s, "last", ORDERS[0])[2]
    dst = (src - 1) % s.T
    r = CV.make_r(n, s.nz, s.dt, s.seed_of_step())
    assert s.code(s.p.convert, src, dst, to_dev(r), None, None, 0, None, sl0, n) is None
    assert not isinstance(s.m.convert(src, dst, r, None, None, 0, sl0=sl0, n=n), int)


def relax(s, sl0, n, first, ntr):
    """the plain form of relax, to the horizontal mean"""
    c = RM.make_c(n, s.nz, s.dt, s.seed_of_step())
    assert s.code(s.p.relax, to_dev(c), None, None, sl0, n, first, ntr) is None
    assert not isinstance(s.m.relax(c, None, sl0=sl0, n=n, first=first, ntr=ntr), int)


def no_negative_zero_from_a_run(s):
    """(behind every step) the plan kernels and the oracle do not agree on the sign of the zero a run returns for a cell that
    held -0.0 and met no flux; the sequences hold none: asserted on the model"""
    if s.op == "run":
        f = s.m.a["f"]
        assert not np.signbit(f[f == 0]).any(), s.at("a -0.0 behind the run", 0, s.ncrms, 0, s.T)


@pytest.mark.parametrize("name,shape,T,dt,sw,seed", CASES, ids=[c[0] for c in CASES])
def test_sequence_with_satadj(mpdata, oracle, name, shape, T, dt, sw, seed):
    s = H.Sequence(mpdata, oracle, Model, UM.make_plan_inputs, name, (shape, T, dt, sw), seed, ref=False,
                   windows=bool(sw.get("tall")), periodic=bool(sw.get("periodic")))
    # (a windowed plan: satadj behind the import, behind a run, behind a satadj, a convert and a relax, and in front of a
    # sediment, which refreshes the seams it marked stale; a periodic one: stale halos, then a run and a block export right
    # behind the call)
    count = s.play(["satadj_ice", "run", "satadj", "convert", "sediment", "satadj_ice", "satadj", "relax", "satadj_ice", "set_boundary",
                    "run", "satadj", "export_block", "satadj_ice", "run", "convert", "export", "satadj", "sediment", "satadj_ice", "run",
                    "import_block", "satadj", "import", "satadj_ice", "satadj_refused"], OPS, STEPS,
                   {"satadj": satadj, "satadj_ice": satadj, "satadj_refused": satadj_refused, "convert": convert, "relax": relax},
                   after=no_negative_zero_from_a_run)
    assert count["satadj"] + count["satadj_ice"] >= 11 and count["run"] >= 4
    assert count["sediment"] >= 2 and count["relax"] >= 1 and count["convert"] >= 2
