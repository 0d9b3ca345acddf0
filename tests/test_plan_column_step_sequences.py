"""GPU tests: seeded call orders that interleave import, block import, block export, run, run of a tracer range,
column_step with every kind of stage set, the single calls cell_add, subside, sediment and vsolve, export and
set_boundary on one resident plan of every non-windowed family -- wave-major fp64 and fp32, odd fp32, two slices per
tile, reference layout --, side by side with the plan model that holds sections 3m, 3n, 3o, 3p and 3q
(tests/subside_model.py, sediment_model.py, vsolve_model.py, cell_add_model.py, column_step_model.py).

Every return code is compared; after every column_step with wp the call's psfc must be the model's on the plan model's
arrays bit for bit (EXACT: the plan's f is bit-identical to the model's); every export and the final one must match.  The
point is the marks across calls: a periodic plan meets column_step with stale and with wrapped halos, the call launches
no wrap and clears the marks, and the run, the subside -- which rewrites the halo slots it finds -- or the read-back that
follows must see wrapped copies of the NEW field wherever the model does."""
import numpy as np
import pytest

import cell_add_model as CM
import column_step_model as QM
import sediment_model as SM
import subside_model as UM
import vsolve_model as VM
from test_plan_cell_add import nan_banded, nan_out
from test_plan_level_stats import BAND, tdt
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
def test_sequence_with_column_step(mpdata, oracle, name, shape, T, dt, sw, seed):
    import torch
    M = mpdata
    ncrms, nx, nz = shape
    M.set_plan_layout(M.LAYOUT_REFERENCE if sw.get("ref") else M.LAYOUT_WAVEMAJOR)
    M.set_f32_odd_ncrms(int(bool(sw.get("odd"))))
    p = M.Plan(*shape, T, dtype=dt)
    assert p.layout == (M.LAYOUT_REFERENCE if name.startswith("ref") else M.LAYOUT_WAVEMAJOR) and p.level_windows == 1
    inp = QM.make_plan_inputs(oracle, shape, T, dt, 100 + seed)
    p.upload(inp["f"], inp["u"], inp["w"], inp["rho"], inp["rhow"], inp["adz"], inp["flux"])
    m = Model(oracle, *shape, T, dt)
    assert m.upload({k: np.array(v, order="F") for k, v in inp.items()}) is None
    rng = np.random.default_rng(seed)
    # (a periodic plan: stale halos behind a run, then a run, a subside and a block export right behind the call)
    script = ["column_step", "run", "column_step", "subside", "column_step", "sediment", "set_boundary", "run_tracers", "column_step",
              "export_block", "column_step", "subside", "export", "column_step", "run", "cell_add", "column_step", "vsolve",
              "import_block", "column_step", "import", "column_step_refused"]
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
            t = torch.empty(M.shapes(n, nx, nz, ntr)["f"], dtype=tdt(dt), device="cuda:0")
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
        elif op == "cell_add":
            s = CM.make_s(n, nx, nz, ntr, dt, seed * 100 + i)
            assert code(p.cell_add, to_dev(s), -0.5, CM.ADD, None, sl0, n, first, ntr) is None
            assert not isinstance(m.cell_add(s, -0.5, CM.ADD, sl0=sl0, n=n, first=first, ntr=ntr), int)
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
        elif op == "column_step_refused":
            kw = QM.make_args(1, nx, nz, 1, dt, seed * 100 + i)
            # a block outside, tracers outside, an unknown mode, half a stage
            bad = [dict(sl0=ncrms, n=1), dict(first=T, ntr=1), dict(mode=2), dict(cc=None)][count[op] % 4]
            a = dict(sl0=0, n=1, first=0, ntr=1, mode=0)
            a.update({k: v for k, v in bad.items() if k in a})
            arrs = dict(kw, **{k: v for k, v in bad.items() if k not in a})
            got = code(p.column_step_device, c=0.75, mode=a["mode"], sl0=a["sl0"], n=a["n"], first_tracer=a["first"], ntracers=a["ntr"],
                       **{k: None if v is None else to_dev(v) for k, v in arrs.items()})
            assert got == M.EINVAL == m.column_step(c=0.75, mode=a["mode"], sl0=a["sl0"], n=a["n"], first=a["first"], ntr=a["ntr"], **arrs)
        else:
            stages = QM.SUBSETS[int(rng.integers(0, 15))] if count[op] % 3 else QM.STAGES
            mode = QM.CLIP if count[op] % 2 else QM.ADD
            c = float(rng.choice([0.75, -0.5, 0.1]))
            kw = QM.make_args(n, nx, nz, ntr, dt, seed * 100 + i, stages)
            sh = M.column_step_shapes(n, nx, nz, ntr)
            dev = {k: nan_banded(kw[k], sh[k])[1] for k in ORDER if k in kw}
            buf = nan_out(sh["psfc"], dt) if "wp" in kw and rng.random() < 0.7 else None
            torch.cuda.synchronize()
            assert code(p.column_step_device, c=c, mode=mode, psfc=buf[2] if buf else None, sl0=sl0, n=n, first_tracer=first, ntracers=ntr,
                        **dev) is None
            p.sync()
            want = m.column_step(c=c, mode=mode, psfc=buf is not None, sl0=sl0, n=n, first=first, ntr=ntr, **kw)
            assert not isinstance(want, int), want
            if buf:
                raw, pristine, view = buf
                assert torch.equal(raw[:BAND], pristine[:BAND]) and torch.equal(raw[-BAND:], pristine[-BAND:])
                assert_bitwise(to_host(view), want, f"{name} step {i}: psfc of block {sl0, n} tracers {first, ntr} stages {stages}")
        assert m.finite()
    i = len(script)
    export()
    assert count["column_step"] >= 8 and count["run"] + count["run_tracers"] >= 3
    assert count["subside"] >= 2 and count["sediment"] >= 1 and count["vsolve"] >= 1 and count["cell_add"] >= 1
    p.close()
