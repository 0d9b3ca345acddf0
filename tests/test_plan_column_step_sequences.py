"""GPU tests: seeded call orders that interleave import, block import, block export, run, run of a tracer range,
column_step with every kind of stage set, the single calls cell_add, subside, sediment and vsolve, export and
set_boundary on one resident plan of every non-windowed family -- wave-major fp64 and fp32, odd fp32, two slices per
tile, reference layout --, side by side with the plan model that holds sections 3m, 3n, 3o, 3p and 3q
(tests/subside_model.py, sediment_model.py, vsolve_model.py, cell_add_model.py, column_step_model.py).

Every return code is compared; after every column_step with wp the call's psfc must be the model's on the plan model's
arrays bit for bit (EXACT: the plan's f is bit-identical to the model's); every export and the final one must match.  The
point is the marks across calls: a periodic plan meets column_step with stale and with wrapped halos, the call launches
no wrap and clears the marks, and the run, the subside -- which rewrites the halo slots it finds -- or the read-back that
follows must see wrapped copies of the NEW field wherever the model does.

The driver and the plain forms of the other ops: tests/plan_harness.py."""
import numpy as np
import pytest

import cell_add_model as CM
import column_step_model as QM
import plan_harness as H
import sediment_model as SM
import subside_model as UM
import vsolve_model as VM
from plan_harness import _defaults
from util import assert_bitwise, to_dev, to_host

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
# name, shape, tracers, dtype, switches, seed
CASES = [("wm-f64-nz28", (5, 4, 28), 2, F64, {}, 81), ("wm-f32-nz28", (6, 3, 28), 2, F32, {}, 82),
         ("f32-odd-nz72", (3, 3, 72), 2, F32, dict(odd=True), 83), ("ref-f64-nz12", (5, 4, 12), 2, F64, dict(ref=True), 84),
         ("ref-f32-odd-nz12", (7, 3, 12), 2, F32, {}, 85)]
STEPS = 24
OPS = ("import", "import_block", "export_block", "run", "run_tracers", "column_step", "cell_add", "subside", "sediment", "vsolve",
       "export", "set_boundary", "column_step_refused")
ORDER = ("s", "cb", "cc", "wp", "lo", "di", "up")


class Model(UM.PlanModelSubside, SM.PlanModelSediment, VM.PlanModelVsolve, CM.PlanModelCellAdd, QM.PlanModelColumnStep):
    pass


def column_step(s, sl0, n, first, ntr):
    """every third call all four stages, else a drawn subset (one draw); c drawn from three factors; the inputs between
    NaN bands; psfc, where wp is given, asked for with probability 0.7 (one draw then), NaN-filled between bands"""
    import torch
    calls = s.count[s.op]
    stages = QM.SUBSETS[int(s.rng.integers(0, 15))] if calls % 3 else QM.STAGES
    mode = QM.CLIP if calls % 2 else QM.ADD
    c = float(s.rng.choice([0.75, -0.5, 0.1]))
    kw = QM.make_args(n, s.nx, s.nz, ntr, s.dt, s.seed_of_step(), stages)
    sh = s.M.column_step_shapes(n, s.nx, s.nz, ntr)
    dev = {k: H.nan_banded(kw[k], sh[k])[1] for k in ORDER if k in kw}
    buf = H.nan_out(sh["psfc"], s.dt) if "wp" in kw and s.rng.random() < 0.7 else None
    torch.cuda.synchronize()
    assert s.code(s.p.column_step_device, c=c, mode=mode, psfc=buf[2] if buf else None, sl0=sl0, n=n, first_tracer=first, ntracers=ntr,
                  **dev) is None
    s.p.sync()
    want = s.m.column_step(c=c, mode=mode, psfc=buf is not None, sl0=sl0, n=n, first=first, ntr=ntr, **kw)
    assert not isinstance(want, int), want
    if buf:
        raw, pristine, view = buf
        assert H.bands_kept(raw, pristine)
        assert_bitwise(to_host(view), want, s.at("psfc", sl0, n, first, ntr) + f" stages {stages}")


def column_step_refused(s, sl0, n, first, ntr):
    M = s.M
    kw = QM.make_args(1, s.nx, s.nz, 1, s.dt, s.seed_of_step())
    # a block outside, tracers outside, an unknown mode, half a stage
    bad = [dict(sl0=s.ncrms, n=1), dict(first=s.T, ntr=1), dict(mode=2), dict(cc=None)][s.count[s.op] % 4]
    a = dict(sl0=0, n=1, first=0, ntr=1, mode=0)
    a.update({k: v for k, v in bad.items() if k in a})
    arrs = dict(kw, **{k: v for k, v in bad.items() if k not in a})
    got = s.code(s.p.column_step_device, c=0.75, mode=a["mode"], sl0=a["sl0"], n=a["n"], first_tracer=a["first"], ntracers=a["ntr"],
                 **{k: None if v is None else to_dev(v) for k, v in arrs.items()})
    assert got == M.EINVAL == s.m.column_step(c=0.75, mode=a["mode"], sl0=a["sl0"], n=a["n"], first=a["first"], ntr=a["ntr"], **arrs)


@pytest.mark.parametrize("name,shape,T,dt,sw,seed", CASES, ids=[c[0] for c in CASES])
def test_sequence_with_column_step(mpdata, oracle, name, shape, T, dt, sw, seed):
    # (the reference layout comes from the case's NAME: "ref-f32-odd-nz12" has no switch and lands there all the same;
    # no case is windowed: the call refuses such plans)
    s = H.Sequence(mpdata, oracle, Model, QM.make_plan_inputs, name, (shape, T, dt, sw), seed, ref=name.startswith("ref"),
                   windows=False)
    # (a periodic plan: stale halos behind a run, then a run, a subside and a block export right behind the call)
    count = s.play(["column_step", "run", "column_step", "subside", "column_step", "sediment", "set_boundary", "run_tracers", "column_step",
                    "export_block", "column_step", "subside", "export", "column_step", "run", "cell_add", "column_step", "vsolve",
                    "import_block", "column_step", "import", "column_step_refused"], OPS, STEPS,
                   {"column_step": column_step, "column_step_refused": column_step_refused, "cell_add": H.plain_cell_add(-0.5)})
    assert count["column_step"] >= 8 and count["run"] + count["run_tracers"] >= 3
    assert count["subside"] >= 2 and count["sediment"] >= 1 and count["vsolve"] >= 1 and count["cell_add"] >= 1
