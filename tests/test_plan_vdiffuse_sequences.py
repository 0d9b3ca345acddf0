"""GPU tests: seeded call orders that interleave import, block import, block export, run, run of a tracer range, vdiffuse
(with and without boundary fluxes), diffuse with cz = 0 (the explicit x half of the pair), vsolve, export and set_boundary
on one resident plan -- wave-major fp64, odd fp32 at nz = 72, the tallest plain plan, a reference-layout plan, a plan that
is PERIODIC from the start, and a windowed plan, which refuses both halves of the pair --, side by side with the plan model
that holds sections 3l, 3o and 3s (tests/diffuse_model.py, vsolve_model.py, vdiffuse_model.py).

Every return code is compared; every export and the final one must match the model bit for bit (EXACT: the plan's f is
bit-identical to the model's).  The point is the marks across calls: a periodic plan meets vdiffuse with stale and with
wrapped halos, and what follows -- a diffuse, which wraps stale halos before it reads them, a run, a read-back -- must see
wrapped copies of the NEW field; the sequence diffuse(cz = 0), vdiffuse is the x-explicit, z-implicit step the call exists
for.  tkh lies between NaN bands with its halo columns NaN, cz with its top level NaN.

The driver and the plain forms of the other ops: tests/plan_harness.py."""
import numpy as np
import pytest

import diffuse_model as DM
import plan_harness as H
import vdiffuse_model as DV
import vsolve_model as VM
from plan_harness import _defaults
from util import to_dev

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
# name, shape, tracers, dtype, switches, seed
CASES = [("wm-f64-nz28", (5, 4, 28), 2, F64, {}, 91), ("f32-odd-nz72", (3, 3, 72), 2, F32, dict(odd=True), 92),
         ("wm-f64-nz238", (5, 3, 238), 2, F64, {}, 93), ("ref-f64-nz12", (5, 3, 12), 2, F64, dict(ref=True), 94),
         ("periodic-f64-nz28-nx11", (5, 11, 28), 2, F64, dict(periodic=True), 95),
         ("tall-f64-nz239", (2, 3, 239), 2, F64, dict(tall=True), 96)]
STEPS = 24
OPS = ("import", "import_block", "export_block", "run", "run_tracers", "vdiffuse", "vdiffuse_fluxes", "diffuse_x", "vsolve", "export",
       "set_boundary", "vdiffuse_refused")


class Model(DM.PlanModelDiffuse, VM.PlanModelVsolve, DV.PlanModelVdiffuse):
    pass


def vdiffuse(s, sl0, n, first, ntr):
    """(both ops, vdiffuse and vdiffuse_fluxes; no draw) the arrays between NaN bands, NaN where the call must not read"""
    import torch
    c = DV.make_coeffs(n, s.nx, s.nz, s.dt, s.seed_of_step(), fluxes=s.op == "vdiffuse_fluxes")
    tkh, cz = np.array(c["tkh"], order="F"), np.array(c["cz"], order="F")
    tkh[:, 0], tkh[:, -1], cz[:, -1] = np.nan, np.nan, np.nan
    sh = s.M.vdiffuse_shapes(n, s.nx, s.nz)
    bufs = {k: H.nan_banded(a, sh[k]) for k, a in (("tkh", tkh), ("cz", cz), ("sb", c["sb"]), ("st", c["st"])) if a is not None}
    orig = {k: raw.clone() for k, (raw, _) in bufs.items()}
    torch.cuda.synchronize()
    got = s.code(s.p.vdiffuse, *(bufs[k][1] if k in bufs else None for k in ("tkh", "cz", "sb", "st")), sl0, n, first, ntr)
    s.p.sync()
    want = s.m.vdiffuse(c["tkh"], c["cz"], c["sb"], c["st"], sl0=sl0, n=n, first=first, ntr=ntr)
    assert got == want, (got, want)
    assert (got == s.M.EUNSUPPORTED) == bool(s.sw.get("tall"))
    for k, (raw, _) in bufs.items():
        assert torch.equal(raw.view(torch.uint8), orig[k].view(torch.uint8)), s.at(k + " changed", sl0, n, first, ntr)


def diffuse_x(s, sl0, n, first, ntr):
    """3l with cz = 0 and no boundary fluxes: the explicit x half; a windowed plan refuses, and the model with it"""
    c = DM.make_coeffs(n, s.nx, s.nz, s.dt, s.seed_of_step(), fluxes=False)
    cz = np.zeros_like(c["cz"])
    got = s.code(s.p.diffuse, to_dev(c["tkh"]), to_dev(c["cx"]), to_dev(cz), None, None, None, sl0, n, first, ntr)
    want = s.m.diffuse(c["tkh"], c["cx"], cz, None, None, sl0=sl0, n=n, first=first, ntr=ntr)
    assert got == (want if isinstance(want, int) else None), (got, want)


def vdiffuse_refused(s, sl0, n, first, ntr):
    M, ncrms, T = s.M, s.ncrms, s.T
    c = DV.make_coeffs(1, s.nx, s.nz, s.dt, s.seed_of_step(), fluxes=False)
    bad = [(ncrms, 1, 0, 1), (0, 1, T, 1), (0, 1, 0, T + 1), (-1, 1, 0, 1)][s.count[s.op] % 4]
    got = s.code(s.p.vdiffuse, to_dev(c["tkh"]), to_dev(c["cz"]), None, None, *bad)
    assert got == M.EINVAL == s.m.vdiffuse(c["tkh"], c["cz"], sl0=bad[0], n=bad[1], first=bad[2], ntr=bad[3])


@pytest.mark.parametrize("name,shape,T,dt,sw,seed", CASES, ids=[c[0] for c in CASES])
def test_sequence_with_vdiffuse(mpdata, oracle, name, shape, T, dt, sw, seed):
    s = H.Sequence(mpdata, oracle, Model, DV.make_plan_inputs, name, (shape, T, dt, sw), seed, ref=bool(sw.get("ref")),
                   windows=bool(sw.get("tall")), periodic=bool(sw.get("periodic")))
    # (vdiffuse behind the import, behind a run, behind itself; the pair diffuse_x, vdiffuse; a periodic plan: stale halos,
    # then a diffuse_x, a run and a block export right behind the call)
    count = s.play(["vdiffuse_fluxes", "run", "diffuse_x", "vdiffuse", "vdiffuse", "diffuse_x", "vsolve", "vdiffuse_fluxes",
                    "set_boundary", "run_tracers", "vdiffuse", "export_block", "diffuse_x", "vdiffuse_fluxes", "run", "vdiffuse",
                    "export", "import_block", "vdiffuse", "import", "vdiffuse_refused"], OPS, STEPS,
                   {"vdiffuse": vdiffuse, "vdiffuse_fluxes": vdiffuse, "diffuse_x": diffuse_x, "vdiffuse_refused": vdiffuse_refused})
    assert count["vdiffuse"] + count["vdiffuse_fluxes"] >= 8 and count["run"] + count["run_tracers"] >= 3
    assert count["diffuse_x"] >= 3 and count["vsolve"] >= 1
