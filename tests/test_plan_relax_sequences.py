"""GPU tests: seeded call orders that interleave import, block import, block export, run, run of a tracer range, relax to
the mean, relax to a target, level_add, cell_add, subside, sediment, vsolve, export and set_boundary on one resident plan
-- wave-major fp64, odd fp32 at nz = 72, a windowed plan, and a plan that is PERIODIC from the start --, side by side with
the plan model that holds sections 3i, 3m, 3n, 3o, 3p and 3r (tests/level_add_model.py, subside_model.py,
sediment_model.py, vsolve_model.py, cell_add_model.py, relax_model.py).

Every return code is compared; after every relax the call's mean must be the model's bit for bit -- without a target it
is a function of every interior value the plan holds for the block at that moment, so each step is compared with the
model right after the call (EXACT: the plan's f is bit-identical to the model's) --; every export and the final one must
match.  The point is the marks across calls: a windowed plan meets relax with fresh seams (behind an import), with stale
ones (behind a run) and with seams a call marked stale (behind another relax, a cell_add, a sediment, a subside or a
vsolve), and the call that follows -- a sediment or a subside, which refresh stale seams before they read a neighbour
level, a run -- must see the NEW field in every copy of a level; a periodic plan meets it with stale and with wrapped
halos, and the run or read-back that follows must see wrapped copies of the NEW field.

The driver and the plain forms of the other ops: tests/plan_harness.py."""
import numpy as np
import pytest

import cell_add_model as CM
import level_add_model as AM
import plan_harness as H
import relax_model as RM
import sediment_model as SM
import subside_model as UM
import vsolve_model as VM
from plan_harness import _defaults
from util import assert_bitwise, to_dev, to_host

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
# name, shape, tracers, dtype, switches, seed
CASES = [("wm-f64-nz28", (5, 4, 28), 2, F64, {}, 81), ("f32-odd-nz72", (3, 3, 72), 2, F32, dict(odd=True), 82),
         ("tall-f64-nz239", (2, 3, 239), 2, F64, dict(tall=True), 83),
         ("periodic-f64-nz28-nx11", (5, 11, 28), 2, F64, dict(periodic=True), 84)]
STEPS = 26
OPS = ("import", "import_block", "export_block", "run", "run_tracers", "relax", "relax_target", "level_add", "cell_add", "subside",
       "sediment", "vsolve", "export", "set_boundary", "relax_refused")


class Model(AM.PlanModelAdd, UM.PlanModelSubside, SM.PlanModelSediment, VM.PlanModelVsolve, CM.PlanModelCellAdd, RM.PlanModelRelax):
    pass


def relax(s, sl0, n, first, ntr):
    """(both ops, relax and relax_target; no draw) c and the target between NaN bands, the mean NaN-filled between
    patterned bands"""
    import torch
    c = RM.make_c(n, s.nz, s.dt, s.seed_of_step())
    tgt = RM.make_target(n, s.nz, ntr, s.dt, s.seed_of_step()) if s.op == "relax_target" else None
    sh = s.M.relax_shapes(n, s.nx, s.nz, ntr)
    craw, cview = H.nan_banded(c, sh["c"])
    traw, tview = H.nan_banded(tgt, sh["target"]) if tgt is not None else (None, None)
    raw, pristine, view = H.nan_out(sh["mean"], s.dt)
    torch.cuda.synchronize()
    assert s.code(s.p.relax, cview, tview, view, sl0, n, first, ntr) is None
    s.p.sync()
    want = s.m.relax(c, tgt, sl0=sl0, n=n, first=first, ntr=ntr)
    assert H.bands_kept(raw, pristine)
    assert_bitwise(to_host(view), want, s.at("mean", sl0, n, first, ntr))


def relax_refused(s, sl0, n, first, ntr):
    M, ncrms, T = s.M, s.ncrms, s.T
    c = RM.make_c(1, s.nz, s.dt, s.seed_of_step())
    bad = [(ncrms, 1, 0, 1), (0, 1, T, 1), (0, 1, 0, T + 1), (-1, 1, 0, 1)][s.count[s.op] % 4]
    got = s.code(s.p.relax, to_dev(c), None, None, *bad)
    assert got == M.EINVAL == s.m.relax(c, None, sl0=bad[0], n=bad[1], first=bad[2], ntr=bad[3])


@pytest.mark.parametrize("name,shape,T,dt,sw,seed", CASES, ids=[c[0] for c in CASES])
def test_sequence_with_relax(mpdata, oracle, name, shape, T, dt, sw, seed):
    # (no case asks for the reference layout)
    s = H.Sequence(mpdata, oracle, Model, RM.make_plan_inputs, name, (shape, T, dt, sw), seed, ref=False,
                   windows=bool(sw.get("tall")), periodic=bool(sw.get("periodic")))
    # (a windowed plan: relax behind the import, behind a run, behind a relax, and in front of a sediment and a subside,
    # which refresh the seams it marked stale; a periodic one: stale halos, then a run and a block export right behind
    # the call)
    count = s.play(["relax", "run", "relax_target", "relax", "sediment", "relax", "subside", "vsolve", "relax_target",
                    "set_boundary", "run_tracers", "relax", "export_block", "relax_target", "run", "relax", "export", "level_add",
                    "relax", "cell_add", "relax_target", "run", "import_block", "relax", "import", "relax_refused"], OPS, STEPS,
                   {"relax": relax, "relax_target": relax, "relax_refused": relax_refused, "cell_add": H.plain_cell_add(0.75)})
    assert count["relax"] + count["relax_target"] >= 10 and count["run"] + count["run_tracers"] >= 4
    assert count["subside"] >= 1 and count["sediment"] >= 1 and count["vsolve"] >= 1 and count["level_add"] >= 1
    assert count["cell_add"] >= 1
