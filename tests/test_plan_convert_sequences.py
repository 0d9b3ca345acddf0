"""GPU tests: seeded call orders that interleave import, block import, block export, run, run of a tracer range, convert,
convert with LIMIT, relax, cell_add, subside, sediment, export and set_boundary on one resident plan of three tracers --
wave-major fp64, odd fp32 at nz = 72, a windowed plan, and a plan that is PERIODIC from the start --, side by side with the
plan model that holds sections 3m, 3n, 3p, 3r and 3t (tests/subside_model.py, sediment_model.py, cell_add_model.py,
relax_model.py, convert_model.py).

Every return code is compared; after every convert the call's dsum must be the model's bit for bit -- it is a function of
every interior value of tracer src the plan holds for the block at that moment, so each step is compared with the model
right after the call (EXACT: the plan's f is bit-identical to the model's) --; every export and the final one must match.
The point is the marks across calls, of TWO tracers at once: a windowed plan meets convert with fresh seams (behind an
import), with stale ones (behind a run) and with seams a call marked stale (behind another convert, a relax, a cell_add, a
sediment or a subside), and the call that follows -- a sediment or a subside, which refresh stale seams before they read
a neighbour level, a run -- must see the NEW field in every copy of a level of BOTH tracers; a periodic plan meets it with
stale and with wrapped halos, and the run or read-back that follows must see wrapped copies of the NEW fields.

The driver and the plain forms of the other ops: tests/plan_harness.py."""
import numpy as np
import pytest

import cell_add_model as CM
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
CASES = [("wm-f64-nz28", (5, 4, 28), 3, F64, {}, 91), ("f32-odd-nz72", (3, 3, 72), 3, F32, dict(odd=True), 92),
         ("tall-f64-nz239", (2, 3, 239), 3, F64, dict(tall=True), 93),
         ("periodic-f64-nz28-nx11", (5, 11, 28), 3, F64, dict(periodic=True), 94)]
STEPS = 28
OPS = ("import", "import_block", "export_block", "run", "run_tracers", "convert", "convert_limit", "relax", "cell_add", "subside",
       "sediment", "export", "set_boundary", "convert_refused")
PAIRS = ((0, 2), (2, 0), (1, 0), (1, 2))


class Model(UM.PlanModelSubside, SM.PlanModelSediment, CM.PlanModelCellAdd, RM.PlanModelRelax, CV.PlanModelConvert):
    pass


def convert(s, sl0, n, first, ntr):
    """(both ops, convert and convert_limit; no draw; the tracer range of the step is not used: the pairs rotate) r, q0 and
    y between NaN bands, q0 and y on every second call, dsum NaN-filled between patterned bands"""
    import torch
    c = s.count["convert"] + s.count["convert_limit"]
    src, dst = PAIRS[c % 4]
    opt = c % 2 == 0
    mode = CV.LIMIT if s.op == "convert_limit" else 0
    r = CV.make_r(n, s.nz, s.dt, s.seed_of_step())
    q0 = CV.make_q0(s.m.a["f"][sl0:sl0 + n, ..., src]) if opt else None
    y = CV.make_y(n, s.nz, s.dt, s.seed_of_step()) if opt else None
    sh = s.M.convert_shapes(n, s.nx, s.nz)
    ins = {k: H.nan_banded(a, sh[k]) for k, a in (("r", r), ("q0", q0), ("y", y)) if a is not None}
    view = lambda k: ins[k][1] if k in ins else None
    raw, pristine, out = H.nan_out(sh["dsum"], s.dt)
    torch.cuda.synchronize()
    assert s.code(s.p.convert, src, dst, view("r"), view("q0"), view("y"), mode, out, sl0, n) is None
    s.p.sync()
    want = s.m.convert(src, dst, r, q0, y, mode, sl0=sl0, n=n)
    assert H.bands_kept(raw, pristine)
    assert_bitwise(to_host(out), want, s.at(f"dsum of pair {src, dst}", sl0, n, first, ntr))


def convert_refused(s, sl0, n, first, ntr):
    M, ncrms, T = s.M, s.ncrms, s.T
    r = CV.make_r(1, s.nz, s.dt, s.seed_of_step())
    # (sl0, n, src, dst, mode)
    bad = [(ncrms, 1, 0, 1, 0), (0, 1, T, 0, 0), (0, 1, 1, 1, 0), (0, 1, 0, 1, 2), (-1, 1, 0, 1, 0)][s.count[s.op] % 5]
    got = s.code(s.p.convert, bad[2], bad[3], to_dev(r), None, None, bad[4], None, bad[0], bad[1])
    assert got == M.EINVAL == s.m.convert(bad[2], bad[3], r, None, None, bad[4], sl0=bad[0], n=bad[1])


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
def test_sequence_with_convert(mpdata, oracle, name, shape, T, dt, sw, seed):
    # (no case asks for the reference layout)
    # (inputs without planted -0.0: tests/test_plan_convert.py has them; here a run would meet them behind any block and mode)
    make_inputs = lambda *a: CV.make_plan_inputs(*a, zeros=False)
    s = H.Sequence(mpdata, oracle, Model, make_inputs, name, (shape, T, dt, sw), seed, ref=False,
                   windows=bool(sw.get("tall")), periodic=bool(sw.get("periodic")))
    # (a windowed plan: convert behind the import, behind a run, behind a convert, and in front of a sediment and a subside,
    # which refresh the seams it marked stale in both tracers; a periodic one: stale halos, then a run and a block export
    # right behind the call)
    count = s.play(["convert", "run", "convert_limit", "convert", "sediment", "convert", "subside", "relax", "convert_limit",
                    "set_boundary", "run_tracers", "convert", "export_block", "convert_limit", "run", "convert", "export", "cell_add",
                    "convert", "sediment", "convert_limit", "run", "import_block", "convert", "subside", "import", "convert",
                    "convert_refused"], OPS, STEPS,
                   {"convert": convert, "convert_limit": convert, "convert_refused": convert_refused, "relax": relax,
                    "cell_add": H.plain_cell_add(0.75)}, after=no_negative_zero_from_a_run)
    assert count["convert"] + count["convert_limit"] >= 12 and count["run"] + count["run_tracers"] >= 4
    assert count["subside"] >= 2 and count["sediment"] >= 2 and count["relax"] >= 1 and count["cell_add"] >= 1
