"""GPU tests: seeded call orders that interleave import, block import, block export, run, run of a tracer range,
column_cond, convert, relax, cell_add, subside, sediment, export and set_boundary on one resident plan of three tracers --
wave-major fp64, odd fp32 at nz = 72, a windowed plan, a plan that is PERIODIC from the start and a plan of 17 columns at
nz = 8 (32 units a group, three batches of columns) --, side by side with the plan model that holds sections 3m, 3n, 3p, 3r,
3t and 3w (tests/subside_model.py, sediment_model.py, cell_add_model.py, relax_model.py, convert_model.py,
column_cond_model.py).

Every return code is compared; after every column_cond the call's outputs must be the model's bit for bit -- they are
functions of every interior value of the condition tracer and the value tracers the plan holds for the block at that
moment, and the bounds are drawn from the model's field at that moment, so that the ties exist (EXACT: the plan's f is
bit-identical to the model's) --; every export and the final one must match.  The point is that the call READS whatever
state the calls in front left and leaves no trace: a windowed plan meets it with fresh seams (behind an import), with
stale ones (behind a run) and with seams a call marked stale (behind a convert, a relax, a cell_add, a sediment or a
subside) and must read the owners' values each time without refreshing; a periodic plan meets it with stale and with
wrapped halos and must not care; and the call that follows -- a run, a sediment or subside that refresh stale seams first, a
read-back that wraps -- must find the marks as they were, or it would skip a refresh or a wrap it owes (or the model, which
the call leaves alone, would not match).

The driver and the plain forms of the other ops: tests/plan_harness.py."""
import numpy as np
import pytest

import cell_add_model as CM
import column_cond_model as CC
import convert_model as CV
import level_cond_model as LC
import plan_harness as H
import relax_model as RM
import sediment_model as SM
import subside_model as UM
from plan_harness import _defaults
from util import assert_bitwise, to_dev, to_host

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
# name, shape, tracers, dtype, switches, seed
CASES = [("wm-f64-nz28", (5, 4, 28), 3, F64, {}, 91), ("f32-odd-nz72", (3, 3, 72), 3, F32, dict(odd=True), 92),
         ("tall-f64-nz239", (2, 3, 239), 3, F64, dict(tall=True), 93),
         ("periodic-f64-nz28-nx11", (5, 11, 28), 3, F64, dict(periodic=True), 94),
         ("wm-f64-nz8-nx17", (3, 17, 8), 3, F64, {}, 95)]
STEPS = 29
OPS = ("import", "import_block", "export_block", "run", "run_tracers", "column_cond", "convert", "relax", "cell_add", "subside",
       "sediment", "export", "set_boundary", "column_cond_refused")
OUTSETS = (CC.OUTPUTS, ("kcnt", "cover"), ("ktop", "kbot"), ("cpath",), ("cpath", "mass"))


class Model(UM.PlanModelSubside, SM.PlanModelSediment, CM.PlanModelCellAdd, RM.PlanModelRelax, CV.PlanModelConvert,
            CC.PlanModelColumnCond):
    pass


def column_cond(s, sl0, n, first, ntr):
    """(no draw; the step's tracer range is the range of the value tracers) the condition tracer, the bounds and the output
    sets rotate with periods 3, 3 (every third call one step on) and 5; lo and hi, drawn from the model's field of the
    block, between NaN bands, the outputs NaN-filled between patterned bands"""
    import torch
    c = s.count["column_cond"] - 1
    tc, bounds, outs = c % 3, CC.BOUNDS[(c + c // 3) % 3], OUTSETS[c % 5]
    lo, hi = CC.call_args(np.asfortranarray(s.m.a["f"][sl0:sl0 + n]), tc, bounds, s.seed_of_step())
    sh = s.M.column_cond_shapes(n, s.nx, s.nz, ntr)
    ins = {k: H.nan_banded(a, sh[k]) for k, a in (("lo", lo), ("hi", hi)) if a is not None}
    bufs = {k: H.nan_out(sh[k], s.dt) for k in outs}
    view = lambda k: ins[k][1] if k in ins else None
    state = (s.p.boundary, s.p.layout)
    torch.cuda.synchronize()
    assert s.code(s.p.column_cond, tc, view("lo"), view("hi"), *[bufs[k][2] if k in bufs else None for k in CC.OUTPUTS], first, sl0,
                  n) is None
    s.p.sync()
    assert (s.p.boundary, s.p.layout) == state
    want = s.m.column_cond(tc, lo, hi, first, ntr, sl0=sl0, n=n, outs=outs)
    assert tuple(want) == tuple(outs)
    for k, w in want.items():
        raw_b, pristine, v = bufs[k]
        assert H.bands_kept(raw_b, pristine)
        assert_bitwise(to_host(v), w, s.at(f"{k} under tracer {tc} ({bounds})", sl0, n, first, ntr))


def column_cond_refused(s, sl0, n, first, ntr):
    import torch
    M, ncrms, T = s.M, s.ncrms, s.T
    nan = lambda *sh: torch.full(sh, float("nan"), dtype=H.tdt(s.dt), device="cuda:0")
    o = {"kcnt": nan(s.nx, 1), "cpath": nan(1, s.nx, 1), "cover": nan(1), "mass": nan(1, 1)}
    lo_h = np.zeros((1, s.nz - 1), s.dt, order="F")
    lo = to_dev(lo_h)
    # (sl0, n, tc, a bound, the outputs, first)
    bad = [(ncrms, 1, 0, True, ("kcnt",), 0), (0, 1, T, True, ("kcnt",), 0), (0, 1, 1, False, ("kcnt",), 0), (0, 1, 0, True, (), 0),
           (0, 1, 0, True, ("cpath",), T), (-1, 1, 0, True, ("kcnt",), 0), (0, 1, 0, True, ("cover",), 0), (0, 1, 0, True, ("kcnt", "mass"), 0)]
    b = bad[(s.count[s.op] - 1) % len(bad)]
    g = lambda k: o[k] if k in b[4] else None
    got = s.code(s.p.column_cond, b[2], lo if b[3] else None, None, g("kcnt"), None, None, g("cpath"), g("cover"), g("mass"), b[5], b[0],
                 b[1])
    assert got == M.EINVAL == s.m.column_cond(b[2], lo_h if b[3] else None, None, b[5], 1, sl0=b[0], n=b[1], outs=b[4])
    torch.cuda.synchronize()
    assert all(torch.isnan(v).all() for v in o.values())


def convert(s, sl0, n, first, ntr):
    """the plain form of convert: r alone, the pairs rotate"""
    src, dst = ((0, 2), (2, 0), (1, 0), (1, 2))[(s.count["convert"] - 1) % 4]
    r = CV.make_r(n, s.nz, s.dt, s.seed_of_step())
    assert s.code(s.p.convert, src, dst, to_dev(r), None, None, 0, None, sl0, n) is None
    assert not isinstance(s.m.convert(src, dst, r, sl0=sl0, n=n), int)


def relax(s, sl0, n, first, ntr):
    """the plain form of relax, to the horizontal mean"""
    c = RM.make_c(n, s.nz, s.dt, s.seed_of_step())
    assert s.code(s.p.relax, to_dev(c), None, None, sl0, n, first, ntr) is None
    assert not isinstance(s.m.relax(c, None, sl0=sl0, n=n, first=first, ntr=ntr), int)


def no_negative_zero_from_a_run(s):
    """(behind every step) the plan kernels and the oracle do not agree on the sign of the zero a run returns for a cell that
    held -0.0 and met no flux (convert_model.plant_negative_zeros; nothing of 3w is involved); the sequences hold none:
    asserted on the model"""
    if s.op in ("run", "run_tracers"):
        f = s.m.a["f"]
        assert not np.signbit(f[f == 0]).any(), s.at("a -0.0 behind the run", 0, s.ncrms, 0, s.T)


@pytest.mark.parametrize("name,shape,T,dt,sw,seed", CASES, ids=[c[0] for c in CASES])
def test_sequence_with_column_cond(mpdata, oracle, name, shape, T, dt, sw, seed):
    # (no case asks for the reference layout; the inputs are those of the level_cond sequences, which these ops are known
    # to keep finite)
    s = H.Sequence(mpdata, oracle, Model, LC.make_plan_inputs, name, (shape, T, dt, sw), seed, ref=False,
                   windows=bool(sw.get("tall")), periodic=bool(sw.get("periodic")))
    # (a windowed plan: column_cond behind the import, behind a run, behind the calls that mark seams stale, and in front of
    # a sediment and a subside, which must still refresh them; a periodic one: stale halos, then a run and a block export
    # right behind the call)
    count = s.play(["column_cond", "run", "column_cond", "column_cond", "sediment", "convert", "column_cond", "subside", "relax",
                    "column_cond", "set_boundary", "run_tracers", "column_cond", "export_block", "column_cond", "run", "column_cond",
                    "export", "cell_add", "column_cond", "sediment", "column_cond", "run", "import_block", "column_cond", "subside",
                    "import", "column_cond", "column_cond_refused"], OPS, STEPS,
                   {"column_cond": column_cond, "column_cond_refused": column_cond_refused, "convert": convert, "relax": relax,
                    "cell_add": H.plain_cell_add(0.75)}, after=no_negative_zero_from_a_run)
    assert count["column_cond"] >= 12 and count["run"] + count["run_tracers"] >= 4
    assert count["subside"] >= 2 and count["sediment"] >= 2 and count["relax"] >= 1 and count["cell_add"] >= 1 and count["convert"] >= 1
