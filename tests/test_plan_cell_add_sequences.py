"""GPU tests: seeded call orders that interleave import, block import, block export, run, run of a tracer range, cell_add,
level_add, subside, sediment, vsolve, export and set_boundary on one resident plan of every family -- wave-major, odd
fp32, reference layout, windowed, windowed odd fp32 --, side by side with the plan model that holds sections 3i, 3m, 3n,
3o and 3p (tests/level_add_model.py, subside_model.py, sediment_model.py, vsolve_model.py, cell_add_model.py).

Every return code is compared; after every cell_add the call's dsum must be the model's on the plan model's arrays bit
for bit (EXACT: the plan's f is bit-identical to the model's); every export and the final one must match.  The point is
the marks across calls: a windowed plan meets cell_add with fresh seams (behind an import), with stale ones (behind a
run) and with seams a call marked stale (behind another cell_add, a sediment, a subside or a vsolve), and the call that
follows -- a sediment or a subside, which refresh stale seams before they read a neighbour level, a run -- must see the
NEW field in every copy of a level; a periodic plan meets it with stale and with wrapped halos, and the run or read-back
that follows must see wrapped copies of the NEW field.

The driver and the plain forms of the other ops: tests/plan_harness.py."""
import numpy as np
import pytest

import cell_add_model as CM
import level_add_model as AM
import plan_harness as H
import sediment_model as SM
import subside_model as UM
import vsolve_model as VM
from plan_harness import _defaults
from util import assert_bitwise, to_dev, to_host

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
# name, shape, tracers, dtype, switches, seed
CASES = [("wm-f64-nz28", (5, 4, 28), 2, F64, {}, 71), ("f32-odd-nz72", (3, 3, 72), 2, F32, dict(odd=True), 72),
         ("ref-f64-nz12", (5, 4, 12), 2, F64, dict(ref=True), 73), ("tall-f64-nz239", (2, 3, 239), 2, F64, dict(tall=True), 74),
         ("tall-f32-odd-nz239", (3, 2, 239), 2, F32, dict(tall=True, odd=True), 75)]
STEPS = 26
OPS = ("import", "import_block", "export_block", "run", "run_tracers", "cell_add", "cell_add_clip", "level_add", "subside", "sediment",
       "vsolve", "export", "set_boundary", "cell_add_refused")


class Model(AM.PlanModelAdd, UM.PlanModelSubside, SM.PlanModelSediment, VM.PlanModelVsolve, CM.PlanModelCellAdd):
    pass


def cell_add(s, sl0, n, first, ntr):
    """(both ops, cell_add and cell_add_clip) c drawn from three factors, then s between NaN bands, then dsum, asked for
    with probability 0.7 (one draw), NaN-filled between patterned bands"""
    import torch
    mode = CM.CLIP if s.op == "cell_add_clip" else CM.ADD
    c = float(s.rng.choice([0.75, -0.5, 0.1]))
    a = CM.make_s(n, s.nx, s.nz, ntr, s.dt, s.seed_of_step())
    sh = s.M.cell_add_shapes(n, s.nx, s.nz, ntr)
    sraw, sview = H.nan_banded(a, sh["s"])
    buf = H.nan_out(sh["dsum"], s.dt) if s.rng.random() < 0.7 else None
    torch.cuda.synchronize()
    assert s.code(s.p.cell_add, sview, c, mode, buf[2] if buf else None, sl0, n, first, ntr) is None
    s.p.sync()
    want = s.m.cell_add(a, c, mode, sl0=sl0, n=n, first=first, ntr=ntr)
    if buf:
        raw, pristine, view = buf
        assert H.bands_kept(raw, pristine)
        assert_bitwise(to_host(view), want, s.at("dsum", sl0, n, first, ntr))


def cell_add_refused(s, sl0, n, first, ntr):
    M, ncrms, T = s.M, s.ncrms, s.T
    a = CM.make_s(1, s.nx, s.nz, 1, s.dt, s.seed_of_step())
    bad = [(ncrms, 1, 0, 1, 0), (0, 1, T, 1, 0), (0, 1, 0, T + 1, 1), (0, 1, 0, 1, 2)][s.count[s.op] % 4]
    got = s.code(s.p.cell_add, to_dev(a), 0.75, bad[4], None, bad[0], bad[1], bad[2], bad[3])
    assert got == M.EINVAL == s.m.cell_add(a, 0.75, bad[4], sl0=bad[0], n=bad[1], first=bad[2], ntr=bad[3])


@pytest.mark.parametrize("name,shape,T,dt,sw,seed", CASES, ids=[c[0] for c in CASES])
def test_sequence_with_cell_add(mpdata, oracle, name, shape, T, dt, sw, seed):
    s = H.Sequence(mpdata, oracle, Model, CM.make_plan_inputs, name, (shape, T, dt, sw), seed, ref=bool(sw.get("ref")),
                   windows=bool(sw.get("tall")))
    # (a windowed plan: cell_add behind the import, behind a run, behind a cell_add, and in front of a sediment and a
    # subside, which refresh the seams it marked stale; a periodic one: stale halos, then a run and a block export right
    # behind the call)
    count = s.play(["cell_add", "run", "cell_add_clip", "cell_add", "sediment", "cell_add", "subside", "vsolve", "cell_add_clip",
                    "set_boundary", "run_tracers", "cell_add", "export_block", "cell_add_clip", "run", "cell_add", "export", "level_add",
                    "cell_add", "run", "import_block", "cell_add", "import", "cell_add_refused"], OPS, STEPS,
                   {"cell_add": cell_add, "cell_add_clip": cell_add, "cell_add_refused": cell_add_refused})
    assert count["cell_add"] + count["cell_add_clip"] >= 10 and count["run"] + count["run_tracers"] >= 4
    assert count["subside"] >= 1 and count["sediment"] >= 1 and count["vsolve"] >= 1 and count["level_add"] >= 1
