"""GPU tests: seeded call orders that interleave import, block import, block export, run, run of a tracer range, sediment,
subside, diffuse, level_add, export and set_boundary on one resident plan of every family -- wave-major, odd fp32,
reference layout, windowed, windowed odd fp32 --, side by side with the plan model that holds sections 3i, 3l, 3m and 3n
(tests/level_add_model.py, diffuse_model.py, subside_model.py, sediment_model.py).

Every return code is compared; after every sediment the call's psfc and pflux must be the model's on the plan model's
arrays bit for bit (EXACT: the plan's f is bit-identical to the model's); every export and the final one must match.  The
point is the marks across calls: a windowed plan meets sediment with fresh seams (behind an import), with stale ones
(behind a run) and with seams a call marked stale (behind another sediment or subside); a periodic plan meets it with stale
and with wrapped halos, and the call that follows -- a diffuse, which reads the halos, a run, a read-back -- must see
wrapped copies of the NEW field.  A windowed plan refuses diffuse, and the model with it.

The driver and the plain forms of the other ops: tests/plan_harness.py."""
import numpy as np
import pytest

import diffuse_model as DM
import level_add_model as AM
import plan_harness as H
import sediment_model as SM
import subside_model as UM
from plan_harness import _defaults
from util import to_dev

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
# name, shape, tracers, dtype, switches, seed
CASES = [("wm-f64-nz28", (5, 4, 28), 2, F64, {}, 61), ("f32-odd-nz72", (3, 3, 72), 2, F32, dict(odd=True), 62),
         ("ref-f64-nz12", (5, 4, 12), 2, F64, dict(ref=True), 63), ("tall-f64-nz239", (2, 3, 239), 2, F64, dict(tall=True), 64),
         ("tall-f32-odd-nz239", (3, 2, 239), 2, F32, dict(tall=True, odd=True), 65)]
STEPS = 22
OPS = ("import", "import_block", "export_block", "run", "run_tracers", "sediment", "subside", "diffuse", "level_add", "export",
       "set_boundary", "sediment_refused")


class Model(AM.PlanModelAdd, DM.PlanModelDiffuse, UM.PlanModelSubside, SM.PlanModelSediment):
    pass


def sediment_refused(s, sl0, n, first, ntr):
    M, ncrms, T = s.M, s.ncrms, s.T
    wp = SM.make_wp(1, s.nx, s.nz, 1, s.dt, s.seed_of_step())
    bad = [(ncrms, 1, 0, 1), (0, 1, T, 1), (0, 1, 0, T + 1)][s.count[s.op] % 3]
    got = s.code(s.p.sediment, to_dev(wp), None, None, bad[0], bad[1], bad[2], bad[3])
    assert got == M.EINVAL == s.m.sediment(wp, sl0=bad[0], n=bad[1], first=bad[2], ntr=bad[3])


@pytest.mark.parametrize("name,shape,T,dt,sw,seed", CASES, ids=[c[0] for c in CASES])
def test_sequence_with_sedimentation(mpdata, oracle, name, shape, T, dt, sw, seed):
    s = H.Sequence(mpdata, oracle, Model, SM.make_plan_inputs, name, (shape, T, dt, sw), seed, ref=bool(sw.get("ref")),
                   windows=bool(sw.get("tall")))
    # (a windowed plan: sediment behind the import, behind a run, behind a sediment and a subside; a periodic one: stale
    # halos, then a diffuse and a block export right behind the call)
    count = s.play(["sediment", "run", "sediment", "sediment", "subside", "sediment", "set_boundary", "run_tracers", "sediment", "diffuse",
                    "sediment", "export_block", "sediment", "export", "level_add", "sediment", "run", "import_block", "sediment", "import",
                    "sediment_refused"], OPS, STEPS, {"sediment": H.checked_sediment, "sediment_refused": sediment_refused})
    assert count["sediment"] >= 9 and count["run"] + count["run_tracers"] >= 3 and count["subside"] >= 1 and count["diffuse"] >= 1
