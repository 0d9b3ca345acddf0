"""GPU tests: seeded call sequences that interleave run, level_add, diffuse, level_stats and column_path on one resident
plan -- a PERIODIC one and a plain (GIVEN) one --, side by side with the plan model that holds sections 3i and 3l
(tests/level_add_model.py PlanModelAdd + tests/diffuse_model.py PlanModelDiffuse).

After every diffuse the call's zflux, and after every step the level statistics and the column integrals of a random
block, must be the models' on the plan model's arrays bit for bit (EXACT: the plan's f is bit-identical to the model's);
at the end the whole export of f and flux must match.  A periodic plan meets the diffusion with stale halos (behind a
run), with fresh ones (behind an export) and with halos that are copies of the old field (behind another diffusion)."""
import numpy as np
import pytest

import column_path_model as CP
import diffuse_model as DM
import level_add_model as AM
import level_stats_model as LM
from oracle import plan_model as PM
from test_plan_column_path import paths
from test_plan_diffuse import banded, tdt
from test_plan_level_stats import stats
from util import assert_bitwise, to_dev, to_host

pytestmark = pytest.mark.gpu
CASES = [("periodic-f64-nz28", (5, 8, 28), 2, np.float64, {}, True, 41), ("given-f32-nz72-odd", (3, 8, 72), 2, np.float32, dict(odd=True), False, 42)]
STEPS = 12


class Model(AM.PlanModelAdd, DM.PlanModelDiffuse):
    pass


@pytest.fixture(autouse=True)
def _defaults(mpdata):
    def reset():
        mpdata.set_tile(-1)
        mpdata.set_wm_flags(0)
        mpdata.set_plan_layout(mpdata.LAYOUT_WAVEMAJOR)
        mpdata.set_variant(mpdata.VARIANT_EXACT)
        mpdata.set_tall_columns(0)
        mpdata.set_f32_odd_ncrms(0)
    reset()
    yield
    reset()


@pytest.mark.parametrize("name,shape,T,dt,sw,periodic,seed", CASES, ids=[c[0] for c in CASES])
def test_sequence_with_diffusion(mpdata, oracle, name, shape, T, dt, sw, periodic, seed):
    import torch
    M = mpdata
    ncrms, nx, nz = shape
    M.set_f32_odd_ncrms(int(bool(sw.get("odd"))))
    p = M.Plan(*shape, T, dtype=dt)
    assert p.layout == M.LAYOUT_WAVEMAJOR
    inp = DM.make_plan_inputs(oracle, shape, T, dt, 100 + seed)
    p.upload(inp["f"], inp["u"], inp["w"], inp["rho"], inp["rhow"], inp["adz"], inp["flux"])
    m = Model(oracle, *shape, T, dt)
    assert m.upload({k: np.array(v, order="F") for k, v in inp.items()}) is None
    if periodic:
        p.set_boundary(M.BOUNDARY_PERIODIC)
        assert m.set_boundary(PM.PERIODIC) is None
    rng = np.random.default_rng(seed)
    script = ["run", "diffuse", "diffuse", "export", "diffuse", "level_add", "diffuse", "run"]
    script += [str(rng.choice(["run", "diffuse", "level_add", "export"])) for _ in range(STEPS - len(script))]
    count = dict.fromkeys(("run", "diffuse", "level_add", "export"), 0)

    def block():
        sl0 = int(rng.integers(0, ncrms))
        n = int(rng.integers(1, ncrms - sl0 + 1))
        if rng.random() < 0.3:
            sl0, n = 0, ncrms
        first = int(rng.integers(0, T))
        return sl0, n, first, int(rng.integers(1, T - first + 1))

    def export():
        t = {k: torch.empty(M.shapes(*shape, T)[k], dtype=tdt(dt), device="cuda:0") for k in ("f", "flux")}
        p.export_device(**t)
        p.sync()
        want = m.export_device()
        for k in t:
            assert_bitwise(to_host(t[k]), want[k], f"{name} step {i}: export of {k}")

    for i, op in enumerate(script):
        count[op] += 1
        sl0, n, first, ntr = block()
        if op == "run":
            p.run(first, ntr)
            assert m.run(first, ntr) is None
        elif op == "export":
            export()
        elif op == "level_add":
            S = float(np.max(np.abs(m.a["f"][sl0:sl0 + n, ..., first:first + ntr])))
            d = np.asfortranarray((rng.uniform(-1.0, 1.0, (n, nz - 1, ntr)) * S).astype(dt))
            p.level_add(to_dev(d), sl0, n, AM.ADD, first)
            assert m.level_add(d, sl0, n, AM.ADD, first) is None
        else:
            c = DM.make_coeffs(n, nx, nz, dt, seed * 100 + i, fluxes=bool(rng.random() < 0.6))
            dev = {k: None if v is None else to_dev(v) for k, v in c.items()}
            zb = banded((ntr, nz, n), dt)
            torch.cuda.synchronize()
            p.diffuse(dev["tkh"], dev["cx"], dev["cz"], dev["sb"], dev["st"], zb[2], sl0, n, first, ntr)
            p.sync()
            assert torch.equal(zb[0][:4096], zb[1][:4096]) and torch.equal(zb[0][-4096:], zb[1][-4096:])
            want = m.diffuse(**c, sl0=sl0, n=n, first=first, ntr=ntr)
            assert_bitwise(to_host(zb[2]), want, f"{name} step {i}: zflux of block {sl0, n} tracers {first, ntr}")
        assert m.finite()
        # the read-only block calls on another block: they see the plan's f as the model holds it
        sl0, n, first, ntr = block()
        F = np.asfortranarray(m.a["f"][sl0:sl0 + n, ..., first:first + ntr])
        got = stats(p, dt, nz - 1, sl0, n, first, ntr, which=("sum",))
        assert_bitwise(got["sum"], LM.level_stats(F)[0], f"{name} step {i} ({op}): level sums of block {sl0, n}")
        gp, gm = paths(M, p, dt, nx, sl0, n, first, ntr)
        wp, wm = CP.column_path(F, inp["rho"][sl0:sl0 + n], inp["adz"][sl0:sl0 + n])
        assert_bitwise(gp, wp, f"{name} step {i} ({op}): column paths of block {sl0, n}")
        assert_bitwise(gm, wm, f"{name} step {i} ({op}): column masses of block {sl0, n}")
    i = len(script)
    export()
    assert count["diffuse"] >= 4 and count["run"] >= 2 and count["level_add"] >= 1
    p.close()
