"""GPU tests: seeded call orders that interleave import, block import, block export, run, run of a tracer range, level_hist,
convert, relax, cell_add, subside, sediment, export and set_boundary on one resident plan of three tracers -- wave-major
fp64, odd fp32 at nz = 72, a windowed plan and a plan that is PERIODIC from the start --, side by side with the plan model
that holds sections 3m, 3n, 3p, 3r, 3t and 3ab (tests/subside_model.py, sediment_model.py, cell_add_model.py,
relax_model.py, convert_model.py, level_hist_model.py).

Every return code is compared; after every level_hist the call's cnt and bsum must be the model's bit for bit.  The edges
are a sorted sample of nb + 1 values of the binned tracer from the model's field of the block at that moment
(LH.sample_edges), so that ties exist (EXACT: the plan's f is bit-identical to the model's); every export and the final one
must match.  The point is that the call READS whatever state the calls in front left and leaves no trace: a windowed plan
meets it with fresh seams, with stale ones and with seams a call marked stale and must read the owners' values each time
without refreshing; a periodic plan meets it with stale and with wrapped halos and must not care; and the call that follows
-- a run, a sediment or subside that refresh stale seams first, a read-back that wraps -- must find the marks as they were.

The driver and the plain forms of the other ops: tests/plan_harness.py."""
import numpy as np
import pytest

import cell_add_model as CM
import convert_model as CV
import level_hist_model as LH
import plan_harness as H
import relax_model as RM
import sediment_model as SM
import subside_model as UM
from test_plan_level_cond_sequences import convert, no_negative_zero_from_a_run, relax
from util import assert_bitwise, to_host

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
# name, shape, tracers, dtype, switches, seed
CASES = [("wm-f64-nz28", (5, 4, 28), 3, F64, {}, 191), ("f32-odd-nz72", (3, 3, 72), 3, F32, dict(odd=True), 192),
         ("tall-f64-nz239", (2, 3, 239), 3, F64, dict(tall=True), 193),
         ("periodic-f64-nz28-nx11", (5, 11, 28), 3, F64, dict(periodic=True), 194)]
STEPS = 29
OPS = ("import", "import_block", "export_block", "run", "run_tracers", "level_hist", "convert", "relax", "cell_add", "subside",
       "sediment", "export", "set_boundary", "level_hist_refused")
OUTS = ("both", "cnt", "bsum")
NBS = (5, 1, 17, 8, 32, 9, 2, 16, 25)


class Model(UM.PlanModelSubside, SM.PlanModelSediment, CM.PlanModelCellAdd, RM.PlanModelRelax, CV.PlanModelConvert,
            LH.PlanModelLevelHist):
    pass


def level_hist(s, sl0, n, first, ntr):
    """(no draw; the step's tracer range is the range of the value tracers) the binned tracer, the bin count and the output
    sets rotate with periods 3, 9 and 3 (every ninth call one step on); the outputs NaN-filled between patterned bands"""
    import torch
    c = s.count["level_hist"] - 1
    tc, nb, outs = c % 3, NBS[c % 9], OUTS[(c // 9 + c) % 3]
    edges = LH.sample_edges(s.m.a["f"][sl0:sl0 + n], tc, nb, s.seed_of_step())
    sh = s.M.level_hist_shapes(n, s.nx, s.nz, nb, ntr)
    bufs = {k: H.nan_out(sh[k], s.dt) for k in ("cnt", "bsum") if outs in ("both", k)}
    out = lambda k: bufs[k][2] if k in bufs else None
    state = (s.p.boundary, s.p.layout)
    torch.cuda.synchronize()
    assert s.code(s.p.level_hist, tc, edges, out("cnt"), out("bsum"), first, nb, sl0, n) is None
    s.p.sync()
    assert (s.p.boundary, s.p.layout) == state
    want = s.m.level_hist(tc, edges, nb, first, ntr, sl0=sl0, n=n, cnt="cnt" in bufs, bsum="bsum" in bufs)
    for k, w in zip(("cnt", "bsum"), want):
        assert (w is None) == (k not in bufs)
        if w is not None:
            raw_b, pristine, v = bufs[k]
            assert H.bands_kept(raw_b, pristine)
            assert_bitwise(to_host(v), w, s.at(f"{k} of tracer {tc} in {nb} bins", sl0, n, first, ntr))


def level_hist_refused(s, sl0, n, first, ntr):
    import torch
    M, ncrms, T = s.M, s.ncrms, s.T
    nan = lambda *sh: torch.full(sh, float("nan"), dtype=H.tdt(s.dt), device="cuda:0")
    cnt, bsum = nan(2, s.nz - 1, 1), nan(1, 2, s.nz - 1, 1)
    ok, desc, nanny = [0.0, 1.0, 2.0], [0.0, 2.0, 1.0], [0.0, float("nan"), 1.0]
    # (sl0, n, tc, edges, cnt, bsum, first)
    bad = [(ncrms, 1, 0, ok, True, True, 0), (0, 1, T, ok, True, True, 0), (0, 1, 1, desc, True, True, 0),
           (0, 1, 0, ok, False, False, 0), (0, 1, 0, ok, True, True, T), (-1, 1, 0, ok, True, True, 0), (0, 1, 2, nanny, True, True, 0)]
    b = bad[(s.count[s.op] - 1) % 7]
    got = s.code(s.p.level_hist, b[2], b[3], cnt if b[4] else None, bsum if b[5] else None, b[6], 2, b[0], b[1])
    assert got == M.EINVAL == s.m.level_hist(b[2], b[3], 2, b[6], 1, sl0=b[0], n=b[1], cnt=b[4], bsum=b[5])
    torch.cuda.synchronize()
    assert torch.isnan(cnt).all() and torch.isnan(bsum).all()


@pytest.mark.parametrize("name,shape,T,dt,sw,seed", CASES, ids=[c[0] for c in CASES])
def test_sequence_with_level_hist(mpdata, oracle, name, shape, T, dt, sw, seed):
    # (no case asks for the reference layout)
    s = H.Sequence(mpdata, oracle, Model, LH.make_plan_inputs, name, (shape, T, dt, sw), seed, ref=False,
                   windows=bool(sw.get("tall")), periodic=bool(sw.get("periodic")))
    count = s.play(["level_hist", "run", "level_hist", "level_hist", "sediment", "convert", "level_hist", "subside", "relax",
                    "level_hist", "set_boundary", "run_tracers", "level_hist", "export_block", "level_hist", "run", "level_hist",
                    "export", "cell_add", "level_hist", "sediment", "level_hist", "run", "import_block", "level_hist", "subside",
                    "import", "level_hist", "level_hist_refused"], OPS, STEPS,
                   {"level_hist": level_hist, "level_hist_refused": level_hist_refused, "convert": convert, "relax": relax,
                    "cell_add": H.plain_cell_add(0.75)}, after=no_negative_zero_from_a_run)
    assert count["level_hist"] >= 12 and count["run"] + count["run_tracers"] >= 4
    assert count["subside"] >= 2 and count["sediment"] >= 2 and count["relax"] >= 1 and count["cell_add"] >= 1 and count["convert"] >= 1
