"""GPU tests: seeded call sequences that interleave run, level_add, diffuse, level_stats and column_path on one resident
plan -- a PERIODIC one and a plain (GIVEN) one --, side by side with the plan model that holds sections 3i and 3l
(tests/level_add_model.py PlanModelAdd + tests/diffuse_model.py PlanModelDiffuse).

After every diffuse the call's zflux, and after every step the level statistics and the column integrals of a random
block, must be the models' on the plan model's arrays bit for bit (EXACT: the plan's f is bit-identical to the model's);
at the end the whole export of f and flux must match.  A periodic plan meets the diffusion with stale halos (behind a
run), with fresh ones (behind an export) and with halos that are copies of the old field (behind another diffusion).

The driver and the plain forms of the other ops: tests/plan_harness.py."""
import numpy as np
import pytest

import column_path_model as CP
import diffuse_model as DM
import level_add_model as AM
import level_stats_model as LM
import plan_harness as H
from plan_harness import _defaults
from test_plan_column_path import paths
from test_plan_level_stats import stats
from util import assert_bitwise, to_dev, to_host

pytestmark = pytest.mark.gpu
CASES = [("periodic-f64-nz28", (5, 8, 28), 2, np.float64, {}, True, 41), ("given-f32-nz72-odd", (3, 8, 72), 2, np.float32, dict(odd=True), False, 42)]
STEPS = 12
OPS = ["run", "diffuse", "level_add", "export"]


class Model(AM.PlanModelAdd, DM.PlanModelDiffuse):
    pass


def diffuse(s, sl0, n, first, ntr):
    """zflux between patterned bands; the flux coefficients are given with probability 0.6 (one draw)"""
    import torch
    c = DM.make_coeffs(n, s.nx, s.nz, s.dt, s.seed_of_step(), fluxes=bool(s.rng.random() < 0.6))
    dev = {k: None if v is None else to_dev(v) for k, v in c.items()}
    zb = H.banded((ntr, s.nz, n), s.dt)
    torch.cuda.synchronize()
    assert s.code(s.p.diffuse, dev["tkh"], dev["cx"], dev["cz"], dev["sb"], dev["st"], zb[2], sl0, n, first, ntr) is None
    s.p.sync()
    assert H.bands_kept(zb[0], zb[1])
    want = s.m.diffuse(**c, sl0=sl0, n=n, first=first, ntr=ntr)
    assert_bitwise(to_host(zb[2]), want, s.at("zflux", sl0, n, first, ntr))


def read_only_calls(s):
    """behind every step, on another block (four more draws): they see the plan's f as the model holds it"""
    sl0, n, first, ntr = s.block()
    F = np.asfortranarray(s.m.a["f"][sl0:sl0 + n, ..., first:first + ntr])
    got = stats(s.p, s.dt, s.nz - 1, sl0, n, first, ntr, which=("sum",))
    assert_bitwise(got["sum"], LM.level_stats(F)[0], f"{s.name} step {s.i} ({s.op}): level sums of block {sl0, n}")
    gp, gm = paths(s.M, s.p, s.dt, s.nx, sl0, n, first, ntr)
    wp, wm = CP.column_path(F, s.inp["rho"][sl0:sl0 + n], s.inp["adz"][sl0:sl0 + n])
    assert_bitwise(gp, wp, f"{s.name} step {s.i} ({s.op}): column paths of block {sl0, n}")
    assert_bitwise(gm, wm, f"{s.name} step {s.i} ({s.op}): column masses of block {sl0, n}")


@pytest.mark.parametrize("name,shape,T,dt,sw,periodic,seed", CASES, ids=[c[0] for c in CASES])
def test_sequence_with_diffusion(mpdata, oracle, name, shape, T, dt, sw, periodic, seed):
    s = H.Sequence(mpdata, oracle, Model, DM.make_plan_inputs, name, (shape, T, dt, sw), seed, ref=False, windows=None,
                   periodic=periodic)
    # (a run here is always one of a tracer range: one op "run", played by the plain form of run_tracers)
    count = s.play(["run", "diffuse", "diffuse", "export", "diffuse", "level_add", "diffuse", "run"], OPS, STEPS,
                   {"run": H.run_tracers, "diffuse": diffuse}, after=read_only_calls)
    assert count["diffuse"] >= 4 and count["run"] >= 2 and count["level_add"] >= 1
