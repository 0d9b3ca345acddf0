"""GPU tests: seeded call orders that interleave import, block import, block export, run, run of a tracer range, level_cov,
convert, relax, cell_add, subside, sediment, export and set_boundary on one resident plan of three tracers -- wave-major
fp64, odd fp32 at nz = 72, a windowed plan, and a plan that is PERIODIC from the start --, side by side with the plan
model that holds sections 3m, 3n, 3p, 3r, 3t and 3u (tests/subside_model.py, sediment_model.py, cell_add_model.py,
relax_model.py, convert_model.py, level_cov_model.py).

Every return code is compared; after every level_cov the call's cov and means must be the model's bit for bit -- they are
functions of every interior value of the two tracers the plan holds for the block at that moment, so each step is compared
with the model right after the call (EXACT: the plan's f is bit-identical to the model's) --; every export and the final
one must match.  The point is that the call READS whatever state the calls in front left and leaves no trace: a windowed
plan meets it with fresh seams (behind an import), with stale ones (behind a run) and with seams a call marked stale
(behind a convert, a relax, a cell_add, a sediment or a subside) and must read the owners' values each time without
refreshing; a periodic plan meets it with stale and with wrapped halos and must not care; and the call that follows -- a
run, a sediment or subside that refresh stale seams first, a read-back that wraps -- must find the marks as they were, or
it would skip a refresh or a wrap it owes (or the model, which the call leaves alone, would not match).

The driver and the plain forms of the other ops: tests/plan_harness.py."""
import numpy as np
import pytest

import cell_add_model as CM
import convert_model as CV
import level_cov_model as LC
import plan_harness as H
import relax_model as RM
import sediment_model as SM
import subside_model as UM
from plan_harness import _defaults
from util import assert_bitwise, to_dev, to_host

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
# name, shape, tracers, dtype, switches, seed
CASES = [("wm-f64-nz28", (5, 4, 28), 3, F64, {}, 91), ("f32-odd-nz72", (3, 3, 72), 3, F32, dict(odd=True), 92),
         ("tall-f64-nz239", (2, 3, 239), 3, F64, dict(tall=True), 93),
         ("periodic-f64-nz28-nx11", (5, 11, 28), 3, F64, dict(periodic=True), 94),
         ("wm-f64-nz8-nx33", (3, 33, 8), 3, F64, {}, 95)]
STEPS = 29
OPS = ("import", "import_block", "export_block", "run", "run_tracers", "level_cov", "convert", "relax", "cell_add", "subside",
       "sediment", "export", "set_boundary", "level_cov_refused")
PAIRS = ((0, 2), (2, 0), (1, 0), (1, 1))
HOWS = list(LC.MEANS)
MEAN_OUTS = ((True, True), (False, False), (True, False), (False, True))


class Model(UM.PlanModelSubside, SM.PlanModelSediment, CM.PlanModelCellAdd, RM.PlanModelRelax, CV.PlanModelConvert,
            LC.PlanModelLevelCov):
    pass


def level_cov(s, sl0, n, first, ntr):
    """(no draw; the tracer range of the step is not used: the pairs, the ways of the means and the mean outputs rotate, with
    periods 4, 5 and 4) ma and mb between NaN bands, the outputs NaN-filled between patterned bands"""
    import torch
    c = s.count["level_cov"] - 1
    ta, tb = PAIRS[c % 4]
    ma, mb, raw = LC.call_args(n, s.nz, s.dt, s.seed_of_step(), HOWS[c % 5])
    means = (False, False) if raw else MEAN_OUTS[(c // 5) % 4]
    sh = s.M.level_cov_shapes(n, s.nx, s.nz)
    ins = {k: H.nan_banded(a, sh[k]) for k, a in (("ma", ma), ("mb", mb)) if a is not None}
    outs = {k: H.nan_out(sh[k], s.dt) for k, on in zip(("cov", "mean_a", "mean_b"), (True,) + means) if on}
    view = lambda k: ins[k][1] if k in ins else None
    out = lambda k: outs[k][2] if k in outs else None
    state = (s.p.boundary, s.p.layout)
    torch.cuda.synchronize()
    assert s.code(s.p.level_cov, ta, tb, out("cov"), view("ma"), view("mb"), LC.RAW if raw else 0, out("mean_a"), out("mean_b"),
                  sl0, n) is None
    s.p.sync()
    assert (s.p.boundary, s.p.layout) == state
    want = s.m.level_cov(ta, tb, ma, mb, LC.RAW if raw else 0, sl0=sl0, n=n, mean_a=means[0], mean_b=means[1])
    for k, w in zip(("cov", "mean_a", "mean_b"), want):
        assert (w is None) == (k not in outs)
        if w is not None:
            raw_b, pristine, v = outs[k]
            assert H.bands_kept(raw_b, pristine)
            assert_bitwise(to_host(v), w, s.at(f"{k} of pair {ta, tb} ({HOWS[c % 5]})", sl0, n, first, ntr))


def level_cov_refused(s, sl0, n, first, ntr):
    import torch
    M, ncrms, T = s.M, s.ncrms, s.T
    cov = torch.full((s.nz - 1, 1), float("nan"), dtype=H.tdt(s.dt), device="cuda:0")
    # (sl0, n, ta, tb, mode, a profile with it)
    bad = [(ncrms, 1, 0, 1, 0, False), (0, 1, T, 0, 0, False), (0, 1, 1, 1, 2, False), (0, 1, 0, 1, 1, True), (-1, 1, 0, 1, 0, False)]
    b = bad[(s.count[s.op] - 1) % 5]
    ma = LC.make_profile(1, s.nz, s.dt, s.seed_of_step()) if b[5] else None
    got = s.code(s.p.level_cov, b[2], b[3], cov, None if ma is None else to_dev(ma), None, b[4], None, None, b[0], b[1])
    assert got == M.EINVAL == s.m.level_cov(b[2], b[3], ma, None, b[4], sl0=b[0], n=b[1])
    torch.cuda.synchronize()
    assert torch.isnan(cov).all()


def convert(s, sl0, n, first, ntr):
    """the plain form of convert: r alone, the pairs rotate"""
    src, dst = ((0, 2), (2, 0), (1, 0), (1, 2))[(s.count["convert"] - 1) % 4]
    r = CV.make_r(n, s.nz, s.dt, s.seed_of_step())
    assert s.code(s.p.convert, src, dst, to_dev(r), None, None, 0, None, sl0, n) is None
    assert not isinstance(s.m.convert(src, dst, r, sl0=sl0, n=n), int)


def relax(s, sl0, n, first, ntr):
    """the plain form of relax, to the horizontal mean"""
    c = RM.make_c(n, s.nz, s.dt, s.seed_of_step())
    assert s.code(s.p.relax, to_dev(c), None, None, sl0, n, first, ntr) is None
    assert not isinstance(s.m.relax(c, None, sl0=sl0, n=n, first=first, ntr=ntr), int)


def no_negative_zero_from_a_run(s):
    """(behind every step) the plan kernels and the oracle do not agree on the sign of the zero a run returns for a cell that
    held -0.0 and met no flux (convert_model.plant_negative_zeros; nothing of 3u is involved); the sequences hold none:
    asserted on the model"""
    if s.op in ("run", "run_tracers"):
        f = s.m.a["f"]
        assert not np.signbit(f[f == 0]).any(), s.at("a -0.0 behind the run", 0, s.ncrms, 0, s.T)


@pytest.mark.parametrize("name,shape,T,dt,sw,seed", CASES, ids=[c[0] for c in CASES])
def test_sequence_with_level_cov(mpdata, oracle, name, shape, T, dt, sw, seed):
    # (no case asks for the reference layout)
    s = H.Sequence(mpdata, oracle, Model, LC.make_plan_inputs, name, (shape, T, dt, sw), seed, ref=False,
                   windows=bool(sw.get("tall")), periodic=bool(sw.get("periodic")))
    # (a windowed plan: level_cov behind the import, behind a run, behind the calls that mark seams stale, and in front of a
    # sediment and a subside, which must still refresh them; a periodic one: stale halos, then a run and a block export
    # right behind the call)
    count = s.play(["level_cov", "run", "level_cov", "level_cov", "sediment", "convert", "level_cov", "subside", "relax", "level_cov",
                    "set_boundary", "run_tracers", "level_cov", "export_block", "level_cov", "run", "level_cov", "export", "cell_add",
                    "level_cov", "sediment", "level_cov", "run", "import_block", "level_cov", "subside", "import", "level_cov",
                    "level_cov_refused"], OPS, STEPS,
                   {"level_cov": level_cov, "level_cov_refused": level_cov_refused, "convert": convert, "relax": relax,
                    "cell_add": H.plain_cell_add(0.75)}, after=no_negative_zero_from_a_run)
    assert count["level_cov"] >= 12 and count["run"] + count["run_tracers"] >= 4
    assert count["subside"] >= 2 and count["sediment"] >= 2 and count["relax"] >= 1 and count["cell_add"] >= 1 and count["convert"] >= 1
