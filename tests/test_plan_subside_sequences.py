"""GPU tests: seeded call orders that interleave import, block import, run, run of a tracer range, subside, level_add,
level_stats, export and set_boundary on one resident plan of every kind -- wave-major, odd fp32, reference layout,
windowed, windowed odd fp32 --, side by side with the plan model that holds sections 3i and 3m (tests/level_add_model.py
PlanModelAdd + tests/subside_model.py PlanModelSubside).

Every return code is compared; after every subside the call's dsum, and after every step the level sums of a random block,
must be the models' on the plan model's arrays bit for bit (EXACT: the plan's f is bit-identical to the model's); every
export and the final one must match.  A windowed plan meets the call with fresh seams (behind an import), with stale ones
(behind a run) and with seams the call itself marked stale (behind another subside); a periodic plan meets it with stale
and with wrapped halos.

The driver and the plain forms of the other ops: tests/plan_harness.py."""
import numpy as np
import pytest

import level_add_model as AM
import level_stats_model as LM
import plan_harness as H
import subside_model as SM
from plan_harness import _defaults
from test_plan_level_stats import stats
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


def subside(s, sl0, n, first, ntr):
    """dsum, asked for with probability 0.7 (one draw, ahead of everything else), between patterned bands"""
    import torch
    cb, cc = SM.make_coeffs(n, s.nz, s.dt, s.seed_of_step())
    db = H.banded((ntr, s.nz - 1, n), s.dt) if s.rng.random() < 0.7 else None
    torch.cuda.synchronize()
    assert s.code(s.p.subside, to_dev(cb), to_dev(cc), None if db is None else db[2], sl0, n, first, ntr) is None
    s.p.sync()
    want = s.m.subside(cb, cc, sl0=sl0, n=n, first=first, ntr=ntr)
    if db is not None:
        assert H.bands_kept(db[0], db[1])
        assert_bitwise(to_host(db[2]), want, s.at("dsum", sl0, n, first, ntr))


def subside_refused(s, sl0, n, first, ntr):
    M, ncrms, T = s.M, s.ncrms, s.T
    cb, cc = SM.make_coeffs(1, s.nz, s.dt, s.seed_of_step())
    bad = [(ncrms, 1, 0, 1), (0, 1, T, 1), (0, 1, 0, T + 1)][s.count[s.op] % 3]
    got = s.code(s.p.subside, to_dev(cb), to_dev(cc), None, bad[0], bad[1], bad[2], bad[3])
    assert got == M.EINVAL == s.m.subside(cb, cc, sl0=bad[0], n=bad[1], first=bad[2], ntr=bad[3])


def level_sums(s):
    """behind every step, a read-only block call on another block (four more draws): it sees the plan's f as the model
    holds it"""
    sl0, n, first, ntr = s.block()
    F = np.asfortranarray(s.m.a["f"][sl0:sl0 + n, ..., first:first + ntr])
    got = stats(s.p, s.dt, s.nz - 1, sl0, n, first, ntr, which=("sum",))
    assert_bitwise(got["sum"], LM.level_stats(F)[0], f"{s.name} step {s.i} ({s.op}): level sums of block {sl0, n}")


@pytest.mark.parametrize("name,shape,T,dt,sw,seed", CASES, ids=[c[0] for c in CASES])
def test_sequence_with_subsidence(mpdata, oracle, name, shape, T, dt, sw, seed):
    s = H.Sequence(mpdata, oracle, Model, SM.make_plan_inputs, name, (shape, T, dt, sw), seed, ref=bool(sw.get("ref")),
                   windows=bool(sw.get("tall")))
    # (a windowed plan: subside behind the import, behind a run, behind a subside; a periodic one: stale and wrapped halos)
    count = s.play(["subside", "run", "subside", "subside", "set_boundary", "run_tracers", "subside", "export", "subside", "level_add",
                    "subside", "run", "import_block", "subside", "import", "subside_refused"], OPS, STEPS,
                   {"subside": subside, "subside_refused": subside_refused}, after=level_sums)
    assert count["subside"] >= 6 and count["run"] + count["run_tracers"] >= 3 and count["level_add"] >= 1
