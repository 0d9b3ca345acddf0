"""GPU tests: seeded call orders that interleave import, block import, block export, run, run of a tracer range,
column_scan in its four modes, combine, subside, sediment, vsolve, export and set_boundary on one resident plan of four
tracers -- wave-major fp64, odd fp32 at nz = 72, a windowed plan, and a plan that is PERIODIC from the start --, side by side
with the plan model that holds sections 3m, 3n, 3o, 3z and 3aa (tests/subside_model.py, sediment_model.py, vsolve_model.py,
combine_model.py, column_scan_model.py).

Every return code is compared; after every column_scan the call's total must be the model's bit for bit -- it is a function
of every interior value of src the plan holds for the block at that moment, so each step is compared with the model right
after the call (EXACT: the plan's f is bit-identical to the model's) --; every export and the final one must match.  The
point is the marks across calls, of dst ALONE: a windowed plan meets the call with fresh seams (behind an import), with
stale ones (behind a run) and with seams a call marked stale (behind another column_scan, a combine, a vsolve, a sediment or
a subside), and the call that follows -- a sediment or a subside, which refresh stale seams before they read a neighbour
level, a run -- must see the NEW field in every copy of a level of dst; the marks of src must be what they were: a run right
behind the call, over all tracers, shows a source whose marks the call cleared or set wrongly.  A periodic plan meets it
with stale and with wrapped halos, and the run or read-back that follows must see wrapped copies of the new dst.

The driver and the plain forms of the other ops: tests/plan_harness.py."""
import numpy as np
import pytest

import column_scan_model as CS
import combine_model as CB
import plan_harness as H
import sediment_model as SM
import subside_model as UM
import test_plan_column_scan as TS
import vsolve_model as VM
from plan_harness import _defaults
from util import assert_bitwise, to_host

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
# name, shape, tracers, dtype, switches, seed
CASES = [("wm-f64-nz28", (5, 4, 28), 4, F64, {}, 91), ("f32-odd-nz72", (3, 3, 72), 4, F32, dict(odd=True), 92),
         ("tall-f64-nz239", (2, 3, 239), 4, F64, dict(tall=True), 93),
         ("periodic-f64-nz28-nx11", (5, 11, 28), 4, F64, dict(periodic=True), 94)]
STEPS = 30
OPS = ("import", "import_block", "export_block", "run", "run_tracers", "scan", "scan_nowgt", "combine", "subside", "sediment", "vsolve",
       "export", "set_boundary", "scan_refused")
# (src, dst, mode): the four modes; dst below, above and on src
LISTS = ((0, 2, 0), (3, 1, CS.DOWN), (1, 1, CS.EXCLUSIVE), (2, 3, CS.DOWN | CS.EXCLUSIVE), (3, 0, CS.DOWN), (2, 2, 0),
         (0, 3, CS.EXCLUSIVE), (1, 0, CS.DOWN | CS.EXCLUSIVE))


class Model(UM.PlanModelSubside, SM.PlanModelSediment, VM.PlanModelVsolve, CB.PlanModelCombine, CS.PlanModelColumnScan):
    pass


def scan(s, sl0, n, first, ntr):
    """(both ops, scan and scan_nowgt; no draw; the tracer range of the step is not used: the lists rotate) wgt between NaN
    bands or absent, total NaN-filled between NaN bands (tests/test_plan_column_scan.py: nan_total).  The source is scaled down first where the field has grown:
    a scan multiplies magnitudes by up to nzm, and thirty steps would leave the floats otherwise."""
    import torch
    c = s.count["scan"] + s.count["scan_nowgt"]
    src, dst, mode = LISTS[c % len(LISTS)]
    wgt = CS.make_wgt(n, s.nz, s.dt, s.seed_of_step()) if s.op == "scan" else None
    S = float(np.max(np.abs(s.m.a["f"][sl0:sl0 + n, ..., src])))
    if S > 4.0:
        coef = np.full((n, s.nz - 1, 1), 1.0 / 2.0 ** np.ceil(np.log2(S)), s.dt, order="F")     # (a power of two: exact)
        assert s.code(s.p.combine, src, (src,), H.to_dev(coef), None, 0, None, sl0, n) is None
        assert not isinstance(s.m.combine(src, (src,), coef, None, 0, sl0=sl0, n=n), int)
    sh = s.M.column_scan_shapes(n, s.nx, s.nz)
    win = H.nan_banded(wgt, sh["wgt"]) if wgt is not None else None
    raw, pristine, out = TS.nan_total(sh["total"], s.dt)
    torch.cuda.synchronize()
    assert s.code(s.p.column_scan, src, dst, win[1] if win else None, out, mode, sl0, n) is None
    s.p.sync()
    want = s.m.column_scan(src, dst, wgt, mode, sl0=sl0, n=n)
    assert TS.total_bands_kept(raw, pristine, s.dt)
    assert_bitwise(to_host(out).reshape(want.shape, order="F"), want, s.at(f"total of src {src} dst {dst} mode {mode}", sl0, n, first, ntr))


def scan_refused(s, sl0, n, first, ntr):
    M, ncrms, T = s.M, s.ncrms, s.T
    # (sl0, n, src, dst, mode)
    bad = [(ncrms, 1, 0, 1, 0), (0, 1, T, 0, 0), (0, 1, 1, T, 0), (0, 1, 0, 1, 4), (-1, 1, 0, 1, 0), (0, 0, 0, 1, 0),
           (0, 1, -1, 0, 8)][s.count[s.op] % 7]
    got = s.code(s.p.column_scan, bad[2], bad[3], None, None, bad[4], bad[0], bad[1])
    assert got == M.EINVAL == s.m.column_scan(bad[2], bad[3], None, bad[4], sl0=bad[0], n=bad[1])


def combine(s, sl0, n, first, ntr):
    """the plain form of combine: a x + b y into a third tracer"""
    dst, src = ((2, (0, 1)), (0, (3, 0)), (1, (2, 3)))[s.count[s.op] % 3]
    coef, _ = CB.call_args(n, s.nz, 2, s.dt, s.seed_of_step(), True, False)
    assert s.code(s.p.combine, dst, src, H.to_dev(coef), None, 0, None, sl0, n) is None
    assert not isinstance(s.m.combine(dst, src, coef, None, 0, sl0=sl0, n=n), int)


@pytest.mark.parametrize("name,shape,T,dt,sw,seed", CASES, ids=[c[0] for c in CASES])
def test_sequence_with_column_scan(mpdata, oracle, name, shape, T, dt, sw, seed):
    # (no case asks for the reference layout: tests/test_plan_column_scan.py has it)
    s = H.Sequence(mpdata, oracle, Model, CS.make_plan_inputs, name, (shape, T, dt, sw), seed, ref=False,
                   windows=bool(sw.get("tall")), periodic=bool(sw.get("periodic")))
    # (a windowed plan: the call behind the import, behind a run, behind another scan, and in front of a sediment and a
    # subside, which refresh the seams it marked stale in dst; a run right behind a call over all tracers: the marks of src;
    # a periodic one: stale halos, then a run and a block export right behind the call)
    count = s.play(["scan", "run", "scan_nowgt", "scan", "sediment", "scan", "subside", "vsolve", "scan_nowgt", "set_boundary",
                    "run_tracers", "scan", "export_block", "scan_nowgt", "run", "scan", "export", "combine", "scan", "sediment",
                    "scan_nowgt", "run", "import_block", "scan", "subside", "scan", "run", "import", "scan_refused"], OPS, STEPS,
                   {"scan": scan, "scan_nowgt": scan, "scan_refused": scan_refused, "combine": combine})
    assert count["scan"] + count["scan_nowgt"] >= 12 and count["run"] + count["run_tracers"] >= 5
    assert count["subside"] >= 2 and count["sediment"] >= 2 and count["vsolve"] >= 1 and count["combine"] >= 1
