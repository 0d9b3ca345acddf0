"""GPU tests: seeded call orders that interleave level_draft with runs, runs of a tracer range, scale_uw, run_uw, imports of
w alone and of u and w, imports of f, level_add, subside, sediment, vsolve, exports and set_boundary on one resident plan of
three tracers -- wave-major fp64, odd fp32 at nz = 72, a windowed plan and a plan that is PERIODIC from the start --, side by
side with the plan model that holds sections 3i, 3j, 3m, 3n, 3o and 3ac (tests/level_add_model.py, scale_uw_model.py,
subside_model.py, sediment_model.py, vsolve_model.py, level_draft_model.py).

Every return code is compared; after every level_draft the call's outputs must be the model's bit for bit.  The point is
that the call READS whatever f AND w the calls in front left and leaves no trace:
  behind scale_uw it must see the SCALED w (a plan's w cannot be read back: this call is the first that shows it directly);
  behind run_uw the plan holds no w: MPDATA_ESTATE, the outputs untouched, until w has been imported whole again -- w alone
    is enough, and the run behind it is still refused until u is back;
  a windowed plan meets it with fresh and with stale seams and must read the owners' values without refreshing; a periodic
    plan meets it with stale and with wrapped halos and must not care; the call that follows must find the marks as they were.
The bounds carry ties (LC.call_args on the model's field of the block at that moment; EXACT: the plan's f is bit-identical
to the model's); the threshold pairs are LD.THRESHOLDS.

The driver and the plain forms of the other ops: tests/plan_harness.py."""
import numpy as np
import pytest

import level_cond_model as LC
import level_draft_model as LD
import plan_harness as H
import scale_uw_model as SU
import sediment_model as SM
import subside_model as UM
import vsolve_model as VM
from oracle import plan_model as PM
from util import assert_bitwise, to_dev, to_host

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
# name, shape, tracers, dtype, switches, seed
CASES = [("wm-f64-nz28", (5, 4, 28), 3, F64, {}, 201), ("f32-odd-nz72", (3, 3, 72), 3, F32, dict(odd=True), 202),
         ("tall-f64-nz239", (2, 3, 239), 3, F64, dict(tall=True), 203),
         ("periodic-f64-nz28-nx11", (5, 11, 28), 3, F64, dict(periodic=True), 204)]
STEPS = 34
OPS = ("import", "import_block", "export_block", "run", "run_tracers", "level_draft", "scale_uw", "run_uw", "import_w", "import_uw",
       "level_add", "subside", "sediment", "vsolve", "export", "set_boundary", "level_draft_refused")
NAMES4 = ("cnt", "wsum", "fsum", "wfsum")
OUTS = (NAMES4, ("cnt", "wsum"), ("fsum", "wfsum"), ("wfsum",), ("cnt", "fsum"))
BOUNDS = ("both", "lo", "hi", None)


class Model(UM.PlanModelSubside, SM.PlanModelSediment, VM.PlanModelVsolve, SU.PlanModelScale, LD.PlanModelLevelDraft):
    pass


def level_draft(s, sl0, n, first, ntr):
    """(no draw; the step's tracer range is the range of the value tracers) the condition tracer (-1 every fourth call), the
    bounds, the thresholds and the output sets rotate with periods 4, 4, 6 and 5; the outputs NaN-filled between patterned
    bands.  Where the model says MPDATA_ESTATE (behind run_uw) so must the plan, and the outputs stay NaN."""
    import torch
    c = s.count["level_draft"] - 1
    tc, bk, thr, outs = (c % 4) - 1, BOUNDS[(c + c // 4) % 4], LD.THRESHOLDS[c % 6], OUTS[c % 5]
    lo, hi = (None, None) if tc < 0 or bk is None else LC.call_args(np.asfortranarray(s.m.a["f"][sl0:sl0 + n]), tc, bk, s.seed_of_step())
    sh = s.M.level_draft_shapes(n, s.nx, s.nz, ntr)
    bufs = {k: H.nan_out(sh[k], s.dt) for k in outs}
    out = lambda k: bufs[k][2] if k in bufs else None
    state = (s.p.boundary, s.p.layout)
    torch.cuda.synchronize()
    got = s.code(s.p.level_draft, tc, None if lo is None else to_dev(lo), None if hi is None else to_dev(hi), thr[0], thr[1], out("cnt"),
                 out("wsum"), out("fsum"), out("wfsum"), first, sl0, n)
    s.p.sync()
    torch.cuda.synchronize()
    assert (s.p.boundary, s.p.layout) == state
    want = s.m.level_draft(tc, lo, hi, thr[0], thr[1], first, ntr, sl0=sl0, n=n, **{k: k in bufs for k in NAMES4})
    if isinstance(want, int):
        assert want == PM.ESTATE and not s.m.have_w and got == s.M.ESTATE, (got, want)
        s.refused_state += 1
        for k, (raw_b, pristine, v) in bufs.items():
            assert H.bands_kept(raw_b, pristine) and torch.isnan(v).all(), k
        return
    assert got is None, got
    s.answered += 1
    for k, w in zip(NAMES4, want):
        assert (w is None) == (k not in bufs)
        if w is not None:
            raw_b, pristine, v = bufs[k]
            assert H.bands_kept(raw_b, pristine)
            assert_bitwise(to_host(v), w, s.at(f"{k} under tracer {tc}, thresholds {thr}", sl0, n, first, ntr))


def level_draft_refused(s, sl0, n, first, ntr):
    import torch
    M, ncrms, T = s.M, s.ncrms, s.T
    nan = lambda *sh: torch.full(sh, float("nan"), dtype=H.tdt(s.dt), device="cuda:0")
    cnt, fsum = nan(3, s.nz - 1, 1), nan(1, 3, s.nz - 1, 1)
    lo = torch.zeros((s.nz - 1, 1), dtype=H.tdt(s.dt), device="cuda:0")
    qnan = float("nan")
    # (sl0, n, tc, lo, wup, wdn, cnt, fsum, first)
    bad = [(ncrms, 1, 0, False, 0.25, -0.25, True, True, 0), (0, 1, T, False, 0.25, -0.25, True, True, 0), (0, 1, -1, True, 0.25, -0.25, True, True, 0),
           (0, 1, 0, False, -0.25, 0.25, True, True, 0), (0, 1, 0, False, 0.25, -0.25, False, False, 0), (0, 1, 0, False, 0.25, -0.25, True, True, T),
           (-1, 1, 0, False, 0.25, -0.25, True, True, 0), (0, 1, 2, True, qnan, -0.25, True, True, 0)]
    b = bad[(s.count[s.op] - 1) % 8]
    got = s.code(s.p.level_draft, b[2], lo if b[3] else None, None, b[4], b[5], cnt if b[6] else None, None, fsum if b[7] else None, None,
                 b[8], b[0], b[1])
    want = s.m.level_draft(b[2], np.zeros((1, s.nz - 1), s.dt, order="F") if b[3] else None, None, b[4], b[5], b[8], 1, sl0=b[0], n=b[1],
                           cnt=b[6], wsum=False, fsum=b[7], wfsum=False)
    assert got == M.EINVAL == want       # (the arguments come before the state: also behind run_uw)
    torch.cuda.synchronize()
    assert torch.isnan(cnt).all() and torch.isnan(fsum).all()


def run(s, sl0, n, first, ntr):
    """behind run_uw the plan holds no velocities: MPDATA_ESTATE from both"""
    got, want = s.code(s.p.run), s.m.run()
    assert got == want and want in (None, PM.ESTATE), (got, want)


def run_tracers(s, sl0, n, first, ntr):
    got, want = s.code(s.p.run, first, ntr), s.m.run(first, ntr)
    assert got == want and want in (None, PM.ESTATE), (got, want)


def _uw(s, shift):
    O = s.oracle
    o = O.make_inputs(s.ncrms, s.nx, s.nz, seed=5000 * s.seed + 10 * s.i + shift, dist=O.DIST_RAW_SIGNED, dtype=s.dt)
    return o["u"], o["w"]


def scale_uw(s, sl0, n, first, ntr):
    """sw always, su every other call: the next level_draft must see the scaled w; refused with MPDATA_ESTATE where the plan
    does not hold what is scaled"""
    c = s.count["scale_uw"] - 1
    sw = SU.make_s(s.shape, s.dt, s.seed_of_step(), n)
    su = SU.make_s(s.shape, s.dt, s.seed_of_step() + 1, n) if c % 2 else None
    got = s.code(s.p.scale_uw, None if su is None else to_dev(su), to_dev(sw), sl0, n)
    want = s.m.scale_uw(su, sw, sl0, n)
    assert got == want and want in (None, PM.ESTATE), (got, want)
    s.scaled += want is None


def run_uw(s, sl0, n, first, ntr):
    u, w = _uw(s, 1)
    assert s.code(s.p.run_uw, to_dev(u), to_dev(w)) is None and s.m.run_uw(u, w) is None
    assert not s.m.have_w and not s.m.have_u


def import_w(s, sl0, n, first, ntr):
    """w alone: enough for level_draft, not for a run behind run_uw"""
    _, w = _uw(s, 2)
    assert s.code(s.p.import_device, w=to_dev(w)) is None and s.m.import_device({"w": w}) is None


def import_uw(s, sl0, n, first, ntr):
    u, w = _uw(s, 3)
    assert s.code(s.p.import_device, u=to_dev(u), w=to_dev(w)) is None and s.m.import_device({"u": u, "w": w}) is None


def no_negative_zero_from_a_run(s):
    """(behind every step) the plan kernels and the oracle do not agree on the sign of the zero a run returns for a cell that
    held -0.0 and met no flux; the sequences hold none: asserted on the model"""
    if s.op in ("run", "run_tracers", "run_uw"):
        f = s.m.a["f"]
        assert not np.signbit(f[f == 0]).any(), s.at("a -0.0 behind the run", 0, s.ncrms, 0, s.T)


@pytest.mark.parametrize("name,shape,T,dt,sw,seed", CASES, ids=[c[0] for c in CASES])
def test_sequence_with_level_draft(mpdata, oracle, name, shape, T, dt, sw, seed):
    # (no case asks for the reference layout)
    s = H.Sequence(mpdata, oracle, Model, LD.make_plan_inputs, name, (shape, T, dt, sw), seed, ref=False,
                   windows=bool(sw.get("tall")), periodic=bool(sw.get("periodic")))
    s.answered = s.refused_state = s.scaled = 0
    count = s.play(["level_draft", "run", "level_draft", "scale_uw", "level_draft", "sediment", "level_draft", "subside", "scale_uw",
                    "level_draft", "set_boundary", "run_tracers", "level_draft", "run_uw", "level_draft", "level_draft_refused", "run",
                    "import_w", "level_draft", "run", "level_draft", "import_uw", "run", "level_draft", "level_add", "level_draft",
                    "vsolve", "import_block", "level_draft", "run_uw", "import_w", "scale_uw", "level_draft", "import_uw"], OPS, STEPS,
                   {"level_draft": level_draft, "level_draft_refused": level_draft_refused, "run": run, "run_tracers": run_tracers,
                    "scale_uw": scale_uw, "run_uw": run_uw, "import_w": import_w, "import_uw": import_uw},
                   after=no_negative_zero_from_a_run)
    assert count["level_draft"] >= 12 and s.answered >= 10 and s.refused_state >= 1 and s.scaled >= 2
    assert count["run"] + count["run_tracers"] >= 4 and count["run_uw"] >= 2 and count["import_w"] >= 2
