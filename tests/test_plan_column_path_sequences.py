"""GPU tests: the seeded call sequences of oracle/plan_model.py with column_path calls (include/mpdata_hip.h 3k) drawn in
between, on an EXACT wave-major plan and a windowed plan, side by side with the plan model with the new call
(tests/column_path_model.py PlanModelPath).

Behind every drawn op of PM.sequences, after the level_add and scale_uw ops that tests/test_plan_level_add_sequences.py and
tests/test_plan_scale_uw_sequences.py insert (run, run_uw, import_block, level_add, scale_uw, set_boundary and the exports
all occur), a seeded coin inserts a column_path with a random block and tracer range.  Its path and mass must be the model's
on the plan model's f, rho and adz bit for bit (EXACT: the plan's f is bit-identical to the model's), and since the call
changes nothing every read-back and every return code of the sequence must still match the model, as must the final whole
export_device and whole download.  Before the first upload the model refuses the call with MPDATA_ESTATE, and so must the
plan."""
import json

import numpy as np
import pytest

import column_path_model as CP
from oracle import plan_model as PM
from plan_harness import _defaults
from test_plan_column_path import paths, same
from test_plan_level_add_sequences import draw_d, with_adds
from test_plan_scale_uw_sequences import ScalePlayer, draw_s, with_scales
from util import assert_bitwise

pytestmark = pytest.mark.gpu

SEQ_KINDS = ("wm32", "tall-239")       # an EXACT wave-major plan and a windowed plan
CASES = [(k, PM.SEEDS[k][0]) for k in SEQ_KINDS]


def with_paths(kind, seed, ops):
    """ops with a column_path behind every op but the closing sync / export_device / download, on a seeded coin"""
    ncrms, nx, nz, T = PM.KINDS[kind]["shape"]
    rng = np.random.default_rng([seed, sorted(PM.KINDS).index(kind), 5])
    out = []
    for i, op in enumerate(ops):
        out.append(dict(op))
        if i < len(ops) - 3 and rng.random() < 0.5:
            sl0 = int(rng.integers(0, ncrms))
            n = int(rng.integers(1, ncrms - sl0 + 1))
            if rng.random() < 0.3:
                sl0, n = 0, ncrms
            first = int(rng.integers(0, T))
            out.append(dict(op="column_path", sl0=sl0, n=n, first=first, ntr=int(rng.integers(1, T - first + 1)),
                            mass=bool(rng.random() < 0.7), flat=bool(rng.random() < 0.5)))
    return out


class PathPlayer(ScalePlayer):
    def __init__(self, M, oracle, kind):
        super().__init__(M, oracle, kind)
        self.model = CP.PlanModelPath(oracle, self.ncrms, self.nx, self.nz, self.T, self.dt)
        self.paths = self.path_refused = 0

    def column_path(self, i, op):
        M = self.M
        sl0, n, first, ntr = op["sl0"], op["n"], op["first"], op["ntr"]
        want = self.model.column_path(sl0, n, first, ntr)
        assert want in (None, PM.ESTATE)
        lead = None if (ntr == 1 and op["flat"]) else ntr
        if want is not None:
            with pytest.raises(M.MpdataError) as e:
                paths(M, self.p, self.dt, self.nx, sl0, n, first, lead, op["mass"])
            assert e.value.code == M.ESTATE, f"op {i} column_path: raised {e.value.code}, the model says MPDATA_ESTATE"
            self.path_refused += 1
            return
        wp, wm = self.model.paths(sl0, n, first, ntr)
        if lead is None:
            wp, wm = np.asfortranarray(wp[..., 0]), np.asfortranarray(wm[..., 0])
        got = paths(M, self.p, self.dt, self.nx, sl0, n, first, lead, op["mass"])
        same(got, (wp, wm), f"op {i} column_path {sl0, n, first, ntr}")
        self.paths += 1

    def play(self, ops):
        M = self.M
        for i, op in enumerate(ops):
            self.at = i
            if op["op"] == "column_path":
                self.column_path(i, op)
                continue
            if op["op"] == "level_add":
                d = draw_d(self.model, op)
                assert self.model.level_add(d, op["sl0"], op["n"], op["mode"], op["first"]) is None and self.model.finite()
                dev = self.dev_in(i, op, {"d": d})["d"]
                self.p.level_add(dev, op["sl0"], op["n"], op["mode"], op["first"])
                self.adds += 1
                continue
            if op["op"] == "scale_uw":
                su, sw = draw_s(self.model, op)
                want = self.model.scale_uw(su, sw, op["sl0"], op["n"])
                assert want in (None, PM.ESTATE) and self.model.finite()
                dev = self.dev_in(i, op, {k: v for k, v in (("su", su), ("sw", sw)) if v is not None})
                if want is None:
                    self.p.scale_uw(dev.get("su"), dev.get("sw"), op["sl0"], op["n"])
                    self.scales += 1
                else:
                    with pytest.raises(M.MpdataError) as e:
                        self.p.scale_uw(dev.get("su"), dev.get("sw"), op["sl0"], op["n"])
                    assert e.value.code == M.ESTATE
                    self.refused += 1
                continue
            want = PM.apply(self.model, self.kind, op, self.oracle)
            err = want if isinstance(want, int) and not isinstance(want, bool) else None
            assert err == op.get("err"), f"op {i}: the model returned {want!r}, the generator recorded {op.get('err')}"
            assert self.model.finite()
            if err is None:
                self.do(i, op, want)
                continue
            n_pending = len(self.pending)
            with pytest.raises(M.MpdataError) as e:
                self.do(i, op, want)
            assert e.value.code == err, f"op {i} {op['op']}: raised {e.value.code}, the model says {err}"
            del self.pending[n_pending:]
        assert not self.pending and not self.alive
        n = len(ops)
        for k in ("f", "flux"):
            assert_bitwise(self.got[n - 2][k], self.got[n - 1][k], f"final export_device against final download, {k}")


@pytest.mark.parametrize("kind,seed", CASES, ids=[f"{k}-{s}" for k, s in CASES])
def test_sequence_with_column_paths(mpdata, oracle, kind, seed):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    ops = with_paths(kind, seed, with_scales(kind, seed, with_adds(kind, seed, PM.sequences(kind, seed, PM.LENGTH, oracle))))
    assert sum(op["op"] == "column_path" for op in ops) >= 4
    pl = PathPlayer(mpdata, oracle, kind)
    try:
        pl.check_kind()
        pl.play(ops)
        print(f"{kind} seed {seed}: {pl.paths} column paths, {pl.path_refused} refused, {pl.scales} scalings, {pl.adds} level_adds")
        assert pl.paths >= 3
    except Exception as e:
        raise AssertionError(f"{kind} seed {seed}: {type(e).__name__} at op {pl.at}: {e}\n"
                             f"ops up to there:\n{json.dumps(ops[:pl.at + 1])}") from e
    finally:
        pl.p.close()
