"""GPU tests: seeded call orders that interleave import, block import, block export, run, run of a tracer range, combine,
combine with CLIP, convert, relax, cell_add, subside, sediment, export and set_boundary on one resident plan of four tracers
-- wave-major fp64, odd fp32 at nz = 72, a windowed plan, and a plan that is PERIODIC from the start --, side by side with
the plan model that holds sections 3m, 3n, 3p, 3r, 3t and 3z (tests/subside_model.py, sediment_model.py, cell_add_model.py,
relax_model.py, convert_model.py, combine_model.py).

Every return code is compared; after every combine the call's sum must be the model's bit for bit -- it is a function of
every interior value of the sources the plan holds for the block at that moment, so each step is compared with the model
right after the call (EXACT: the plan's f is bit-identical to the model's) --; every export and the final one must match.
The point is the marks across calls, of dst ALONE: a windowed plan meets combine with fresh seams (behind an import), with
stale ones (behind a run) and with seams a call marked stale (behind another combine, a convert, a relax, a cell_add, a
sediment or a subside), and the call that follows -- a sediment or a subside, which refresh stale seams before they read a
neighbour level, a run -- must see the NEW field in every copy of a level of dst; the marks of a SOURCE must be what they
were: a run right behind the call, over all tracers, shows a source whose marks the call cleared or set wrongly.  A periodic
plan meets it with stale and with wrapped halos, and the run or read-back that follows must see wrapped copies of the new dst.

The driver and the plain forms of the other ops: tests/plan_harness.py."""
import numpy as np
import pytest

import cell_add_model as CM
import combine_model as CB
import convert_model as CV
import plan_harness as H
import relax_model as RM
import sediment_model as SM
import subside_model as UM
from plan_harness import _defaults
from util import assert_bitwise, to_dev, to_host

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
# name, shape, tracers, dtype, switches, seed
CASES = [("wm-f64-nz28", (5, 4, 28), 4, F64, {}, 91), ("f32-odd-nz72", (3, 3, 72), 4, F32, dict(odd=True), 92),
         ("tall-f64-nz239", (2, 3, 239), 4, F64, dict(tall=True), 93),
         ("periodic-f64-nz28-nx11", (5, 11, 28), 4, F64, dict(periodic=True), 94)]
STEPS = 30
OPS = ("import", "import_block", "export_block", "run", "run_tracers", "combine", "combine_clip", "convert", "relax", "cell_add",
       "subside", "sediment", "export", "set_boundary", "combine_refused")
# (dst, src, coef, c0): every class of the source count; dst below, above and among the sources
LISTS = ((2, (0, 2), True, True), (0, (1,), False, False), (3, (0, 1, 2, 3), True, False), (1, (), False, True),
         (0, (3, 2, 1, 0, 3), True, True), (3, (3, 3), False, True), (1, (0, 2, 3), True, True), (2, (0, 1, 2, 3, 3, 2, 1, 0), True, False))


class Model(UM.PlanModelSubside, SM.PlanModelSediment, CM.PlanModelCellAdd, RM.PlanModelRelax, CV.PlanModelConvert, CB.PlanModelCombine):
    pass


def combine(s, sl0, n, first, ntr):
    """(both ops, combine and combine_clip; no draw; the tracer range of the step is not used: the lists rotate) coef and c0
    between NaN bands, sum NaN-filled between patterned bands"""
    import torch
    c = s.count["combine"] + s.count["combine_clip"]
    dst, src, co, cz = LISTS[c % len(LISTS)]
    mode = CB.CLIP if s.op == "combine_clip" else 0
    coef, c0 = CB.call_args(n, s.nz, len(src), s.dt, s.seed_of_step(), co, cz)
    sh = s.M.combine_shapes(n, s.nx, s.nz, len(src))
    ins = {k: H.nan_banded(a, sh[k]) for k, a in (("coef", coef), ("c0", c0)) if a is not None}
    view = lambda k: ins[k][1] if k in ins else None
    raw, pristine, out = H.nan_out(sh["sum"], s.dt)
    torch.cuda.synchronize()
    assert s.code(s.p.combine, dst, src, view("coef"), view("c0"), mode, out, sl0, n) is None
    s.p.sync()
    want = s.m.combine(dst, src, coef, c0, mode, sl0=sl0, n=n)
    assert H.bands_kept(raw, pristine)
    assert_bitwise(to_host(out), want, s.at(f"sum of dst {dst} src {src}", sl0, n, first, ntr))


def combine_refused(s, sl0, n, first, ntr):
    M, ncrms, T = s.M, s.ncrms, s.T
    # (sl0, n, dst, src, mode)
    bad = [(ncrms, 1, 0, (1,), 0), (0, 1, T, (0,), 0), (0, 1, 1, (0, T), 0), (0, 1, 0, (1,), 2), (-1, 1, 0, (1,), 0), (0, 1, 0, (), 0),
           (0, 1, 0, (1,) * 9, 0)][s.count[s.op] % 7]
    got = s.code(s.p.combine, bad[2], bad[3], None, None, bad[4], None, bad[0], bad[1])
    assert got == M.EINVAL == s.m.combine(bad[2], bad[3], None, None, bad[4], sl0=bad[0], n=bad[1])


def convert(s, sl0, n, first, ntr):
    """the plain form of convert, r alone"""
    src, dst = ((0, 2), (3, 1), (1, 0))[s.count[s.op] % 3]
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
    held -0.0 and met no flux (CV.plant_negative_zeros); the sequences hold none: asserted on the model"""
    if s.op in ("run", "run_tracers"):
        f = s.m.a["f"]
        assert not np.signbit(f[f == 0]).any(), s.at("a -0.0 behind the run", 0, s.ncrms, 0, s.T)


@pytest.mark.parametrize("name,shape,T,dt,sw,seed", CASES, ids=[c[0] for c in CASES])
def test_sequence_with_combine(mpdata, oracle, name, shape, T, dt, sw, seed):
    # (no case asks for the reference layout; inputs without planted -0.0, NaN or infinities: tests/test_plan_combine.py has
    # them; here a run would meet them behind any block and mode)
    make_inputs = lambda *a: CB.make_plan_inputs(*a, zeros=False)
    s = H.Sequence(mpdata, oracle, Model, make_inputs, name, (shape, T, dt, sw), seed, ref=False,
                   windows=bool(sw.get("tall")), periodic=bool(sw.get("periodic")))
    # (a windowed plan: combine behind the import, behind a run, behind a combine, and in front of a sediment and a subside,
    # which refresh the seams it marked stale in dst; a run right behind a call over all tracers: the sources' marks; a
    # periodic one: stale halos, then a run and a block export right behind the call)
    count = s.play(["combine", "run", "combine_clip", "combine", "sediment", "combine", "subside", "relax", "combine_clip",
                    "set_boundary", "run_tracers", "combine", "export_block", "combine_clip", "run", "combine", "export", "cell_add",
                    "combine", "sediment", "combine_clip", "run", "import_block", "combine", "subside", "convert", "combine", "run",
                    "import", "combine_refused"], OPS, STEPS,
                   {"combine": combine, "combine_clip": combine, "combine_refused": combine_refused, "convert": convert, "relax": relax,
                    "cell_add": H.plain_cell_add(0.75)}, after=no_negative_zero_from_a_run)
    assert count["combine"] + count["combine_clip"] >= 12 and count["run"] + count["run_tracers"] >= 5
    assert count["subside"] >= 2 and count["sediment"] >= 2 and count["relax"] >= 1 and count["cell_add"] >= 1 and count["convert"] >= 1
