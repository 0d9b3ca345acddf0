"""GPU tests: seeded call orders that interleave import, block import, block export, run, run of a tracer range, vsolve,
sediment, subside, diffuse, level_add, export and set_boundary on one resident plan of every family -- wave-major, odd
fp32, reference layout, windowed, windowed odd fp32 --, side by side with the plan model that holds sections 3i, 3l, 3m, 3n
and 3o (tests/level_add_model.py, diffuse_model.py, subside_model.py, sediment_model.py, vsolve_model.py).

Every return code is compared; every export and the final one must match the model bit for bit (EXACT: the plan's f is
bit-identical to the model's).  The point is the marks across calls: a windowed plan meets vsolve with fresh seams (behind
an import), with stale ones (behind a run) and with seams a call marked stale (behind another vsolve, a sediment or a
subside), and the subside or sediment that follows must refresh the seams vsolve left stale; a periodic plan meets it
with stale and with wrapped halos, and the call that follows -- a diffuse, which reads the halos, a run, a read-back --
must see wrapped copies of the NEW field.  A windowed plan refuses diffuse, and the model with it.

The driver and the plain forms of the other ops: tests/plan_harness.py."""
import numpy as np
import pytest

import diffuse_model as DM
import level_add_model as AM
import plan_harness as H
import sediment_model as SM
import subside_model as UM
import vsolve_model as VM
from plan_harness import _defaults
from util import to_dev

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
# name, shape, tracers, dtype, switches, seed
CASES = [("wm-f64-nz28", (5, 4, 28), 2, F64, {}, 61), ("f32-odd-nz72", (3, 3, 72), 2, F32, dict(odd=True), 62),
         ("ref-f64-nz12", (5, 4, 12), 2, F64, dict(ref=True), 63), ("tall-f64-nz239", (2, 3, 239), 2, F64, dict(tall=True), 64),
         ("tall-f32-odd-nz239", (3, 2, 239), 2, F32, dict(tall=True, odd=True), 65)]
STEPS = 26
OPS = ("import", "import_block", "export_block", "run", "run_tracers", "vsolve", "sediment", "subside", "diffuse", "level_add", "export",
       "set_boundary", "vsolve_refused")


class Model(AM.PlanModelAdd, DM.PlanModelDiffuse, UM.PlanModelSubside, SM.PlanModelSediment, VM.PlanModelVsolve):
    pass


def vsolve(s, sl0, n, first, ntr):
    """lo, di, up between NaN bands; every byte of the three buffers must come back unchanged"""
    import torch
    c = VM.make_coeffs(n, s.nz, s.dt, s.seed_of_step())
    sh = s.M.vsolve_shapes(n, s.nz)
    bufs = [H.nan_banded(a, sh[k]) for a, k in zip(c, ("lo", "di", "up"))]
    orig = [raw.clone() for raw, _ in bufs]
    torch.cuda.synchronize()
    assert s.code(s.p.vsolve, bufs[0][1], bufs[1][1], bufs[2][1], sl0, n, first, ntr) is None
    s.p.sync()
    for (raw, _), o in zip(bufs, orig):
        assert torch.equal(raw.view(torch.uint8), o.view(torch.uint8))
    assert s.m.vsolve(*c, sl0=sl0, n=n, first=first, ntr=ntr) is None


def vsolve_refused(s, sl0, n, first, ntr):
    M, ncrms, T = s.M, s.ncrms, s.T
    c = VM.make_coeffs(1, s.nz, s.dt, s.seed_of_step())
    bad = [(ncrms, 1, 0, 1), (0, 1, T, 1), (0, 1, 0, T + 1)][s.count[s.op] % 3]
    got = s.code(s.p.vsolve, *(to_dev(a) for a in c), bad[0], bad[1], bad[2], bad[3])
    assert got == M.EINVAL == s.m.vsolve(*c, sl0=bad[0], n=bad[1], first=bad[2], ntr=bad[3])


@pytest.mark.parametrize("name,shape,T,dt,sw,seed", CASES, ids=[c[0] for c in CASES])
def test_sequence_with_vertical_solves(mpdata, oracle, name, shape, T, dt, sw, seed):
    s = H.Sequence(mpdata, oracle, Model, SM.make_plan_inputs, name, (shape, T, dt, sw), seed, ref=bool(sw.get("ref")),
                   windows=bool(sw.get("tall")))
    # (a windowed plan: vsolve behind the import, behind a run, behind a vsolve, a subside and a sediment, and each of
    # those behind a vsolve; a periodic one: stale halos, then a diffuse and a block export right behind the call)
    count = s.play(["vsolve", "run", "vsolve", "vsolve", "subside", "vsolve", "sediment", "vsolve", "set_boundary", "run_tracers", "vsolve",
                    "diffuse", "vsolve", "export_block", "vsolve", "export", "level_add", "vsolve", "run", "import_block", "vsolve", "import",
                    "vsolve_refused", "sediment"], OPS, STEPS,
                   {"vsolve": vsolve, "vsolve_refused": vsolve_refused, "sediment": H.checked_sediment})
    assert count["vsolve"] >= 10 and count["run"] + count["run_tracers"] >= 3 and count["subside"] >= 1 and count["diffuse"] >= 1
    assert count["sediment"] >= 2
