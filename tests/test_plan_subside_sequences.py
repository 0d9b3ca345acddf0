"""GPU tests: seeded call orders that interleave import, block import, run, run of a tracer range, subside, level_add,
level_stats, export and set_boundary on one resident plan of every kind -- wave-major, odd fp32, reference layout,
windowed, windowed odd fp32 --, side by side with the plan model that holds sections 3i and 3m (tests/level_add_model.py
PlanModelAdd + tests/subside_model.py PlanModelSubside).

Every return code is compared; after every subside the call's dsum, and after every step the level sums of a random block,
must be the models' on the plan model's arrays bit for bit (EXACT: the plan's f is bit-identical to the model's); every
export and the final one must match.  A windowed plan meets the call with fresh seams (behind an import), with stale ones
(behind a run) and with seams the call itself marked stale (behind another subside); a periodic plan meets it with stale
and with wrapped halos."""
import numpy as np
import pytest

import level_add_model as AM
import level_stats_model as LM
import subside_model as SM
from oracle import plan_model as PM
from test_plan_level_stats import BAND, banded, stats, tdt
from util import assert_bitwise, to_dev, to_host

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
# name, shape, tracers, dtype, switches, seed
CASES = [("wm-f64-nz28", (5, 4, 28), 2, F64, {}, 51), ("f32-odd-nz72", (3, 3, 72), 2, F32, dict(odd=True), 52),
         ("ref-f64-nz12", (5, 4, 12), 2, F64, dict(ref=True), 53), ("tall-f64-nz239", (2, 3, 239), 2, F64, dict(tall=True), 54),
         ("tall-f32-odd-nz239", (3, 2, 239), 2, F32, dict(tall=True, odd=True), 55)]
STEPS = 20
OPS = ("import", "import_block", "run", "run_tracers", "subside", "level_add", "export", "set_boundary", "subside_refused")


class Model(AM.PlanModelAdd, SM.PlanModelSubside):
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
def test_sequence_with_subsidence(mpdata, oracle, name, shape, T, dt, sw, seed):
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
    assert m.upload({k: np.array(v, order="F") for k, v in inp.items()}) is None
    rng = np.random.default_rng(seed)
    # (a windowed plan: subside behind the import, behind a run, behind a subside; a periodic one: stale and wrapped halos)
    script = ["subside", "run", "subside", "subside", "set_boundary", "run_tracers", "subside", "export", "subside", "level_add",
              "subside", "run", "import_block", "subside", "import", "subside_refused"]
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
        elif op == "subside_refused":
            cb, cc = SM.make_coeffs(1, nz, dt, seed * 100 + i)
            bad = [(ncrms, 1, 0, 1), (0, 1, T, 1), (0, 1, 0, T + 1)][count[op] % 3]
            got = code(p.subside, to_dev(cb), to_dev(cc), None, bad[0], bad[1], bad[2], bad[3])
            assert got == M.EINVAL == m.subside(cb, cc, sl0=bad[0], n=bad[1], first=bad[2], ntr=bad[3])
        else:
            cb, cc = SM.make_coeffs(n, nz, dt, seed * 100 + i)
            db = banded((ntr, nz - 1, n), dt) if rng.random() < 0.7 else None
            torch.cuda.synchronize()
            assert code(p.subside, to_dev(cb), to_dev(cc), None if db is None else db[2], sl0, n, first, ntr) is None
            p.sync()
            want = m.subside(cb, cc, sl0=sl0, n=n, first=first, ntr=ntr)
            if db is not None:
                assert torch.equal(db[0][:BAND], db[1][:BAND]) and torch.equal(db[0][-BAND:], db[1][-BAND:])
                assert_bitwise(to_host(db[2]), want, f"{name} step {i}: dsum of block {sl0, n} tracers {first, ntr}")
        assert m.finite()
        # a read-only block call on another block: it sees the plan's f as the model holds it
        sl0, n, first, ntr = block()
        F = np.asfortranarray(m.a["f"][sl0:sl0 + n, ..., first:first + ntr])
        got = stats(p, dt, nz - 1, sl0, n, first, ntr, which=("sum",))
        assert_bitwise(got["sum"], LM.level_stats(F)[0], f"{name} step {i} ({op}): level sums of block {sl0, n}")
    i = len(script)
    export()
    assert count["subside"] >= 6 and count["run"] + count["run_tracers"] >= 3 and count["level_add"] >= 1
    p.close()
