"""GPU tests: the seeded call sequences of oracle/plan_model.py with per-instance velocity scalings (include/mpdata_hip.h
3j) drawn in between, on an EXACT plan and on the plan model with the new call (tests/scale_uw_model.py PlanModelScale)
side by side.

A plan's u and w cannot be read back; what a scaling did -- and what it could leave behind: a phantom half that no longer
follows its instance, a touched partner of a split pair, a window scaled twice or not at all, a flag that moved -- shows
only in what LATER runs return.  So behind every drawn op of PM.sequences, after the level_add ops that
tests/test_plan_level_add_sequences.py inserts (run, run_uw, import_block, level_add, set_boundary and the exports all
occur), a seeded coin inserts a scale_uw with a random block and su, sw or both, and every read-back and every return code
of the sequence must still match the model bit for bit, as must the final whole export_device and whole download.  After
run_uw the model refuses the scaling with MPDATA_ESTATE, and so must the plan.  The factors have magnitude <= 1
(tests/scale_uw_model.py make_s), so the velocities stay in the stable range; they are device tensors that must be
bit-identical afterwards."""
import json

import numpy as np
import pytest

import scale_uw_model as SM
from oracle import plan_model as PM
from plan_harness import _defaults
from test_plan_level_add_sequences import AddPlayer, draw_d, with_adds
from util import assert_bitwise

pytestmark = pytest.mark.gpu

SEQ_KINDS = ("wm32", "ref", "ks-72", "f32-28", "f32-odd-28", "tall-239", "tall-f32-odd-239")   # one per kind family
CASES = [(k, PM.SEEDS[k][0]) for k in SEQ_KINDS]


def with_scales(kind, seed, ops):
    """ops with a scale_uw behind every op but the closing sync / export_device / download, on a seeded coin"""
    ncrms = PM.KINDS[kind]["shape"][0]
    rng = np.random.default_rng([seed, sorted(PM.KINDS).index(kind), 4])
    out = []
    for i, op in enumerate(ops):
        out.append(dict(op))
        if i < len(ops) - 3 and rng.random() < 0.5:
            sl0 = int(rng.integers(0, ncrms))
            n = int(rng.integers(1, ncrms - sl0 + 1))
            if rng.random() < 0.3:
                sl0, n = 0, ncrms
            out.append(dict(op="scale_uw", sl0=sl0, n=n, which=("both", "u", "w")[int(rng.integers(0, 3))], seed=int(rng.integers(1 << 30))))
    return out


def draw_s(model, op):
    shape = model.dims[:3]
    su = SM.make_s(shape, model.dtype, op["seed"], op["n"]) if op["which"] in ("both", "u") else None
    sw = SM.make_s(shape, model.dtype, op["seed"] + 1, op["n"]) if op["which"] in ("both", "w") else None
    return su, sw


class ScalePlayer(AddPlayer):
    def __init__(self, M, oracle, kind):
        super().__init__(M, oracle, kind)
        self.model = SM.PlanModelScale(oracle, self.ncrms, self.nx, self.nz, self.T, self.dt)
        self.scales = self.refused = 0

    def play(self, ops):
        M = self.M
        for i, op in enumerate(ops):
            self.at = i
            if op["op"] == "level_add":
                d = draw_d(self.model, op)
                assert self.model.level_add(d, op["sl0"], op["n"], op["mode"], op["first"]) is None and self.model.finite()
                dev = self.dev_in(i, op, {"d": d})["d"]      # (compared with d at the next synchronisation)
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
                    assert e.value.code == M.ESTATE, f"op {i} scale_uw: raised {e.value.code}, the model says MPDATA_ESTATE"
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
def test_sequence_with_scalings(mpdata, oracle, kind, seed):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    ops = with_scales(kind, seed, with_adds(kind, seed, PM.sequences(kind, seed, PM.LENGTH, oracle)))
    assert sum(op["op"] == "scale_uw" for op in ops) >= 4
    pl = ScalePlayer(mpdata, oracle, kind)
    try:
        pl.check_kind()
        pl.play(ops)
        print(f"{kind} seed {seed}: {pl.scales} scalings, {pl.refused} refused, {pl.adds} level_adds")
        assert pl.scales + pl.refused >= 4 and pl.scales >= 1
    except Exception as e:
        raise AssertionError(f"{kind} seed {seed}: {type(e).__name__} at op {pl.at}: {e}\n"
                             f"ops up to there:\n{json.dumps(ops[:pl.at + 1])}") from e
    finally:
        pl.p.close()
