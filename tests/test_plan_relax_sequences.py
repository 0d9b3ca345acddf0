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
halos, and the run or read-back that follows must see wrapped copies of the NEW field."""
import numpy as np
import pytest

import cell_add_model as CM
import level_add_model as AM
import relax_model as RM
import sediment_model as SM
import subside_model as UM
import vsolve_model as VM
from oracle import plan_model as PM
from test_plan_relax import nan_banded, nan_out
from test_plan_level_stats import BAND, tdt
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


@pytest.mark.parametrize("name,shape,T,dt,sw,seed", CASES, ids=[c[0] for c in CASES])
def test_sequence_with_relax(mpdata, oracle, name, shape, T, dt, sw, seed):
    import torch
    M = mpdata
    ncrms, nx, nz = shape
    M.set_tall_columns(int(bool(sw.get("tall"))))
    M.set_f32_odd_ncrms(int(bool(sw.get("odd"))))
    p = M.Plan(*shape, T, dtype=dt)
    assert p.layout == M.LAYOUT_WAVEMAJOR
    assert (p.level_windows > 1) == bool(sw.get("tall"))
    inp = RM.make_plan_inputs(oracle, shape, T, dt, 100 + seed)
    p.upload(inp["f"], inp["u"], inp["w"], inp["rho"], inp["rhow"], inp["adz"], inp["flux"])
    m = Model(oracle, *shape, T, dt)
    assert m.upload({k: np.array(v, order="F") for k, v in inp.items()}) is None
    if sw.get("periodic"):
        p.set_boundary(M.BOUNDARY_PERIODIC)
        assert m.set_boundary(PM.PERIODIC) is None
    rng = np.random.default_rng(seed)
    # (a windowed plan: relax behind the import, behind a run, behind a relax, and in front of a sediment and a subside,
    # which refresh the seams it marked stale; a periodic one: stale halos, then a run and a block export right behind
    # the call)
    script = ["relax", "run", "relax_target", "relax", "sediment", "relax", "subside", "vsolve", "relax_target",
              "set_boundary", "run_tracers", "relax", "export_block", "relax_target", "run", "relax", "export", "level_add",
              "relax", "cell_add", "relax_target", "run", "import_block", "relax", "import", "relax_refused"]
    script += [str(rng.choice(OPS)) for _ in range(STEPS - len(script))]
    count = dict.fromkeys(OPS, 0)

    def block():
        sl0 = int(rng.integers(0, ncrms))
        n = int(rng.integers(1, ncrms - sl0 + 1))
        if rng.random() < 0.3:
            sl0, n = 0, ncrms
        first = int(rng.integers(0, T))
        return sl0, n, first, int(rng.integers(1, T - first + 1))

    def fresh_f(n, ntr, s):
        per = [oracle.make_inputs(n, nx, nz, seed=1000 * seed + 10 * s + t, dist=oracle.DIST_RAW_SIGNED, dtype=dt)["f"] - dt(0.5)
               for t in range(ntr)]
        return per[0] if ntr == 1 else np.asfortranarray(np.stack(per, axis=-1))

    def code(fn, *a, **kw):
        """the call's return code: None, or the code of the MpdataError it raises"""
        try:
            fn(*a, **kw)
        except M.MpdataError as e:
            return e.code
        return None

    def export():
        t = {k: torch.empty(M.shapes(*shape, T)[k], dtype=tdt(dt), device="cuda:0") for k in ("f", "flux")}
        assert code(p.export_device, **t) is None
        p.sync()
        want = m.export_device()
        for k in t:
            assert_bitwise(to_host(t[k]), want[k], f"{name} step {i}: export of {k}")

    for i, op in enumerate(script):
        count[op] += 1
        sl0, n, first, ntr = block()
        if op == "run":
            assert code(p.run) is None and m.run() is None
        elif op == "run_tracers":
            assert code(p.run, first, ntr) is None and m.run(first, ntr) is None
        elif op == "export":
            export()
        elif op == "export_block":
            sh = M.shapes(n, nx, nz, ntr)["f"]
            t = torch.empty(sh, dtype=tdt(dt), device="cuda:0")
            assert code(p.export_block, sl0, f=t, first_tracer=first) is None
            p.sync()
            want = m.export_block(sl0, n, ("f",), first, ntr)["f"]
            assert_bitwise(to_host(t).reshape(want.shape, order="F"), want, f"{name} step {i}: export of block {sl0, n}")
        elif op == "set_boundary":
            mode = 1 - m.boundary
            assert code(p.set_boundary, mode) is None and m.set_boundary(mode) is None
            assert p.boundary == mode
        elif op == "import":
            f = fresh_f(ncrms, ntr, i)
            assert code(p.import_device, f=to_dev(f), first_tracer=first) is None
            assert m.import_device({"f": f}, first, ntr) is None
        elif op == "import_block":
            f = fresh_f(n, ntr, i)
            assert code(p.import_block, sl0, f=to_dev(f), first_tracer=first) is None
            assert m.import_block(sl0, n, {"f": f}, first, ntr) is None
        elif op == "level_add":
            S = float(np.max(np.abs(m.a["f"][sl0:sl0 + n, ..., first:first + ntr])))
            d = np.asfortranarray((rng.uniform(-1.0, 1.0, (n, nz - 1, ntr)) * S).astype(dt))
            assert code(p.level_add, to_dev(d), sl0, n, AM.ADD, first) is None
            assert m.level_add(d, sl0, n, AM.ADD, first) is None
        elif op == "cell_add":
            s = CM.make_s(n, nx, nz, ntr, dt, seed * 100 + i)
            assert code(p.cell_add, to_dev(s), 0.75, CM.ADD, None, sl0, n, first, ntr) is None
            assert not isinstance(m.cell_add(s, 0.75, CM.ADD, sl0=sl0, n=n, first=first, ntr=ntr), int)
        elif op == "subside":
            cb, cc = UM.make_coeffs(n, nz, dt, seed * 100 + i)
            assert code(p.subside, to_dev(cb), to_dev(cc), None, sl0, n, first, ntr) is None
            assert m.subside(cb, cc, sl0=sl0, n=n, first=first, ntr=ntr) is not None
        elif op == "sediment":
            wp = SM.make_wp(n, nx, nz, ntr, dt, seed * 100 + i)
            assert code(p.sediment, to_dev(wp), None, None, sl0, n, first, ntr) is None
            assert not isinstance(m.sediment(wp, sl0=sl0, n=n, first=first, ntr=ntr), int)
        elif op == "vsolve":
            lo, di, up = VM.make_coeffs(n, nz, dt, seed * 100 + i)
            assert code(p.vsolve, to_dev(lo), to_dev(di), to_dev(up), sl0, n, first, ntr) is None
            assert m.vsolve(lo, di, up, sl0=sl0, n=n, first=first, ntr=ntr) is None
        elif op == "relax_refused":
            c = RM.make_c(1, nz, dt, seed * 100 + i)
            bad = [(ncrms, 1, 0, 1), (0, 1, T, 1), (0, 1, 0, T + 1), (-1, 1, 0, 1)][count[op] % 4]
            got = code(p.relax, to_dev(c), None, None, *bad)
            assert got == M.EINVAL == m.relax(c, None, sl0=bad[0], n=bad[1], first=bad[2], ntr=bad[3])
        else:
            c = RM.make_c(n, nz, dt, seed * 100 + i)
            tgt = RM.make_target(n, nz, ntr, dt, seed * 100 + i) if op == "relax_target" else None
            sh = M.relax_shapes(n, nx, nz, ntr)
            craw, cview = nan_banded(c, sh["c"])
            traw, tview = nan_banded(tgt, sh["target"]) if tgt is not None else (None, None)
            raw, pristine, view = nan_out(sh["mean"], dt)
            torch.cuda.synchronize()
            assert code(p.relax, cview, tview, view, sl0, n, first, ntr) is None
            p.sync()
            want = m.relax(c, tgt, sl0=sl0, n=n, first=first, ntr=ntr)
            assert torch.equal(raw[:BAND], pristine[:BAND]) and torch.equal(raw[-BAND:], pristine[-BAND:])
            assert_bitwise(to_host(view), want, f"{name} step {i}: mean of block {sl0, n} tracers {first, ntr}")
        assert m.finite()
    i = len(script)
    export()
    assert count["relax"] + count["relax_target"] >= 10 and count["run"] + count["run_tracers"] >= 4
    assert count["subside"] >= 1 and count["sediment"] >= 1 and count["vsolve"] >= 1 and count["level_add"] >= 1
    assert count["cell_add"] >= 1
    p.close()
