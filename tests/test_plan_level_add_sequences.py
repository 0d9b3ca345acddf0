"""GPU tests: the seeded call sequences of oracle/plan_model.py with per-level increments (include/mpdata_hip.h 3i) drawn
in between, on an EXACT plan and on the plan model with the new call (tests/level_add_model.py PlanModelAdd) side by side.

The increment is the first plan call besides run and import that writes f in place; what it could leave behind -- a
halo or seam byte that no longer tells the truth, a phantom half that no longer follows its instance, a touched partner
of a split pair -- shows only in what LATER calls return.  So behind every drawn op of PM.sequences (tests/
test_plan_sequences.py plays them plain) a seeded coin inserts a level_add with a random mode, block and tracer range, and
every read-back and every return code of the sequence must still match the model bit for bit (f with its halo columns,
flux at all nz levels), as must the final whole export_device and whole download.  |f| stays bounded: a d is drawn no
larger than the largest |f| the model holds in the block at that point, and the model caps the steps.  d is a device
tensor that must be bit-identical afterwards."""
import json

import numpy as np
import pytest

import level_add_model as AM
from oracle import plan_model as PM
from plan_harness import _defaults
from test_plan_sequences import Player
from util import assert_bitwise

pytestmark = pytest.mark.gpu

SEQ_KINDS = ("wm32", "ref", "f32-odd-28", "tall-239", "tall-f32-odd-239")
CASES = [(k, s) for k in SEQ_KINDS for s in PM.SEEDS[k]]


def with_adds(kind, seed, ops):
    """ops with a level_add behind every op but the closing sync / export_device / download, on a seeded coin"""
    ncrms, nx, nz, T = PM.KINDS[kind]["shape"]
    rng = np.random.default_rng([seed, sorted(PM.KINDS).index(kind), 3])
    out = []
    for i, op in enumerate(ops):
        out.append(dict(op))
        if i < len(ops) - 3 and rng.random() < 0.6:
            sl0 = int(rng.integers(0, ncrms))
            n = int(rng.integers(1, ncrms - sl0 + 1))
            if rng.random() < 0.3:
                sl0, n = 0, ncrms
            first = int(rng.integers(0, T))
            out.append(dict(op="level_add", sl0=sl0, n=n, mode=int(rng.integers(0, 2)), first=first,
                            ntr=int(rng.integers(1, T - first + 1)), seed=int(rng.integers(1 << 30)), flat=bool(rng.random() < 0.5)))
    return out


def draw_d(model, op):
    """d (n, nzm, ntr) -- (n, nzm) for one tracer where op['flat'] -- uniform in (-S, S), S the largest |f| the model holds in
    the block and tracers now"""
    sl0, n, first, ntr = op["sl0"], op["n"], op["first"], op["ntr"]
    nzm = model.dims[2] - 1
    S = float(np.max(np.abs(model.a["f"][sl0:sl0 + n, ..., first:first + ntr])))
    d = (np.random.default_rng(op["seed"]).uniform(-1.0, 1.0, (n, nzm, ntr)) * S).astype(model.dtype)
    return np.asfortranarray(d[..., 0] if ntr == 1 and op["flat"] else d)


class AddPlayer(Player):
    def __init__(self, M, oracle, kind):
        super().__init__(M, oracle, kind, "exact")
        self.model = AM.PlanModelAdd(oracle, self.ncrms, self.nx, self.nz, self.T, self.dt)
        self.adds = 0

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
def test_sequence_with_level_adds(mpdata, oracle, kind, seed):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    ops = with_adds(kind, seed, PM.sequences(kind, seed, PM.LENGTH, oracle))
    assert sum(op["op"] == "level_add" for op in ops) >= 4
    pl = AddPlayer(mpdata, oracle, kind)
    try:
        pl.check_kind()
        pl.play(ops)
        assert pl.adds >= 4
    except Exception as e:
        raise AssertionError(f"{kind} seed {seed}: {type(e).__name__} at op {pl.at}: {e}\n"
                             f"ops up to there:\n{json.dumps(ops[:pl.at + 1])}") from e
    finally:
        pl.p.close()
