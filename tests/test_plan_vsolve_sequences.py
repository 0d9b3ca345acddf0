"""GPU tests: seeded call orders that interleave import, block import, block export, run, run of a tracer range, vsolve,
sediment, subside, diffuse, level_add, export and set_boundary on one resident plan of every family -- wave-major, odd
fp32, reference layout, windowed, windowed odd fp32 --, side by side with the plan model that holds sections 3i, 3l, 3m, 3n
and 3o (tests/level_add_model.py, diffuse_model.py, subside_model.py, sediment_model.py, vsolve_model.py).

Every return code is compared; every export and the final one must match the model bit for bit (EXACT: the plan's f is
bit-identical to the model's).  The point is the marks across calls: a windowed plan meets vsolve with fresh seams (behind
an import), with stale ones (behind a run) and with seams a call marked stale (behind another vsolve, a sediment or a
subside), and the subside or sediment that follows must refresh the seams vsolve left stale; a periodic plan meets it
with stale and with wrapped halos, and the call that follows -- a diffuse, which reads the halos, a run, a read-back --
must see wrapped copies of the NEW field.  A windowed plan refuses diffuse, and the model with it."""
import numpy as np
import pytest

import diffuse_model as DM
import level_add_model as AM
import sediment_model as SM
import subside_model as UM
import vsolve_model as VM
from test_plan_level_stats import BAND, tdt
from test_plan_sediment import nan_banded, nan_out
from util import assert_bitwise, to_dev, to_host

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
def test_sequence_with_vertical_solves(mpdata, oracle, name, shape, T, dt, sw, seed):
    import torch
    M = mpdata
    ncrms, nx, nz = shape
    M.set_plan_layout(M.LAYOUT_REFERENCE if sw.get("ref") else M.LAYOUT_WAVEMAJOR)
    M.set_tall_columns(int(bool(sw.get("tall"))))
    M.set_f32_odd_ncrms(int(bool(sw.get("odd"))))
    p = M.Plan(*shape, T, dtype=dt)
    assert p.layout == (M.LAYOUT_REFERENCE if sw.get("ref") else M.LAYOUT_WAVEMAJOR)
    assert (p.level_windows > 1) == bool(sw.get("tall"))
    inp = SM.make_plan_inputs(oracle, shape, T, dt, 100 + seed)
    p.upload(inp["f"], inp["u"], inp["w"], inp["rho"], inp["rhow"], inp["adz"], inp["flux"])
    m = Model(oracle, *shape, T, dt)
    m.windowed = bool(sw.get("tall"))
    assert m.upload({k: np.array(v, order="F") for k, v in inp.items()}) is None
    rng = np.random.default_rng(seed)
    # (a windowed plan: vsolve behind the import, behind a run, behind a vsolve, a subside and a sediment, and each of
    # those behind a vsolve; a periodic one: stale halos, then a diffuse and a block export right behind the call)
    script = ["vsolve", "run", "vsolve", "vsolve", "subside", "vsolve", "sediment", "vsolve", "set_boundary", "run_tracers", "vsolve",
              "diffuse", "vsolve", "export_block", "vsolve", "export", "level_add", "vsolve", "run", "import_block", "vsolve", "import",
              "vsolve_refused", "sediment"]
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
        elif op == "subside":
            cb, cc = UM.make_coeffs(n, nz, dt, seed * 100 + i)
            assert code(p.subside, to_dev(cb), to_dev(cc), None, sl0, n, first, ntr) is None
            assert m.subside(cb, cc, sl0=sl0, n=n, first=first, ntr=ntr) is not None
        elif op == "diffuse":
            c = DM.make_coeffs(n, nx, nz, dt, seed * 100 + i)
            dev = {k: None if v is None else to_dev(v) for k, v in c.items()}
            got = code(p.diffuse, dev["tkh"], dev["cx"], dev["cz"], dev["sb"], dev["st"], None, sl0, n, first, ntr)
            want = m.diffuse(c["tkh"], c["cx"], c["cz"], c["sb"], c["st"], sl0=sl0, n=n, first=first, ntr=ntr)
            assert got == (want if isinstance(want, int) else None), (got, want)
            assert (got == M.EUNSUPPORTED) == bool(sw.get("tall"))
        elif op == "vsolve_refused":
            c = VM.make_coeffs(1, nz, dt, seed * 100 + i)
            bad = [(ncrms, 1, 0, 1), (0, 1, T, 1), (0, 1, 0, T + 1)][count[op] % 3]
            got = code(p.vsolve, *(to_dev(a) for a in c), bad[0], bad[1], bad[2], bad[3])
            assert got == M.EINVAL == m.vsolve(*c, sl0=bad[0], n=bad[1], first=bad[2], ntr=bad[3])
        elif op == "vsolve":
            c = VM.make_coeffs(n, nz, dt, seed * 100 + i)
            sh = M.vsolve_shapes(n, nz)
            bufs = [nan_banded(a, sh[k]) for a, k in zip(c, ("lo", "di", "up"))]
            orig = [raw.clone() for raw, _ in bufs]
            torch.cuda.synchronize()
            assert code(p.vsolve, bufs[0][1], bufs[1][1], bufs[2][1], sl0, n, first, ntr) is None
            p.sync()
            for (raw, _), o in zip(bufs, orig):
                assert torch.equal(raw.view(torch.uint8), o.view(torch.uint8))
            assert m.vsolve(*c, sl0=sl0, n=n, first=first, ntr=ntr) is None
        else:
            wp = SM.make_wp(n, nx, nz, ntr, dt, seed * 100 + i)
            outs = [k for k in ("psfc", "pflux") if rng.random() < 0.7]
            sh = M.sediment_shapes(n, nx, nz, ntr)
            wraw, wview = nan_banded(wp, sh["wp"])
            bufs = {k: nan_out(sh[k], dt) for k in outs}
            torch.cuda.synchronize()
            assert code(p.sediment, wview, bufs["psfc"][2] if "psfc" in bufs else None, bufs["pflux"][2] if "pflux" in bufs else None,
                        sl0, n, first, ntr) is None
            p.sync()
            want = dict(zip(("psfc", "pflux"), m.sediment(wp, sl0=sl0, n=n, first=first, ntr=ntr)))
            for k, (raw, pristine, view) in bufs.items():
                assert torch.equal(raw[:BAND], pristine[:BAND]) and torch.equal(raw[-BAND:], pristine[-BAND:])
                assert_bitwise(to_host(view), want[k], f"{name} step {i}: {k} of block {sl0, n} tracers {first, ntr}")
        assert m.finite()
    i = len(script)
    export()
    assert count["vsolve"] >= 10 and count["run"] + count["run_tracers"] >= 3 and count["subside"] >= 1 and count["diffuse"] >= 1
    assert count["sediment"] >= 2
    p.close()
