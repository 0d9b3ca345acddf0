"""GPU tests: seeded call orders that interleave import, block import, block export, run, run of a tracer range, nonneg,
relax, level_add, cell_add, subside, sediment, export and set_boundary on one resident plan -- wave-major fp64, odd fp32 at
nz = 72, a windowed plan, and a plan that is PERIODIC from the start --, side by side with the plan model that holds
sections 3i, 3m, 3n, 3p, 3r and 3x (tests/level_add_model.py, subside_model.py, sediment_model.py, cell_add_model.py,
relax_model.py, nonneg_model.py).

Every return code is compared; after every nonneg the call's sum and nneg must be the model's bit for bit -- they are
functions of every interior value the plan holds for the block at that moment, so each step is compared with the model
right after the call (EXACT: the plan's f is bit-identical to the model's) --; every export and the final one must match
(zeros as zeros: class Sequence below).
The point is the marks across calls: a windowed plan meets nonneg with fresh seams (behind an import), with stale ones
(behind a run) and with seams a call marked stale (behind another nonneg, a cell_add, a sediment, a subside or a relax), and
the call that follows -- a sediment or a subside, which refresh stale seams before they read a neighbour level, a run --
must see the NEW field in every copy of a level; a periodic plan meets it with stale and with wrapped halos, and the run
or read-back that follows must see wrapped copies of the NEW field.  The imports, level_add, cell_add and subside put the
negative cells back that the call removes; over a sequence the calls must meet keep rows, fix rows and zero rows, which
the test counts on the model.

The driver and the plain forms of the other ops: tests/plan_harness.py."""
import numpy as np
import pytest

import cell_add_model as CM
import level_add_model as AM
import nonneg_model as NM
import plan_harness as H
import relax_model as RM
import sediment_model as SM
import subside_model as UM
from plan_harness import _defaults
from util import assert_bitwise, to_dev, to_host

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
# name, shape, tracers, dtype, switches, seed
CASES = [("wm-f64-nz28", (5, 4, 28), 2, F64, {}, 91), ("f32-odd-nz72", (3, 3, 72), 2, F32, dict(odd=True), 92),
         ("tall-f64-nz239", (2, 3, 239), 2, F64, dict(tall=True), 93),
         ("periodic-f64-nz28-nx11", (5, 11, 28), 2, F64, dict(periodic=True), 94)]
STEPS = 26
OPS = ("import", "import_block", "export_block", "run", "run_tracers", "nonneg", "relax", "level_add", "cell_add", "subside",
       "sediment", "export", "set_boundary", "nonneg_refused")


class Model(AM.PlanModelAdd, UM.PlanModelSubside, SM.PlanModelSediment, CM.PlanModelCellAdd, RM.PlanModelRelax, NM.PlanModelNonneg):
    pass


class Sequence(H.Sequence):
    """H.Sequence whose read-backs compare zeros as zeros: the fields here hold -0.0 (the keep rows keep theirs) and exact
    zeros (the call makes them), and behind a run of such a field a zero may come out of the advection kernels with the
    other sign than the oracle's (the table of section 1: the hardware max / min order -0 below +0), which is
    no matter of this call.  Everything else of a read-back, and every sum and nneg, is compared bit for bit."""

    def export(self):
        import torch
        t = {k: torch.empty(self.M.shapes(*self.shape, self.T)[k], dtype=H.tdt(self.dt), device="cuda:0") for k in ("f", "flux")}
        assert self.code(self.p.export_device, **t) is None
        self.p.sync()
        want = self.m.export_device()
        for k in t:
            assert_bitwise(AM.canon(to_host(t[k])), AM.canon(want[k]), f"{self.name} step {self.i}: export of {k}")


def export(s, sl0, n, first, ntr):
    s.export()


def export_block(s, sl0, n, first, ntr):
    import torch
    t = torch.empty(s.M.shapes(n, s.nx, s.nz, ntr)["f"], dtype=H.tdt(s.dt), device="cuda:0")
    assert s.code(s.p.export_block, sl0, f=t, first_tracer=first) is None
    s.p.sync()
    want = s.m.export_block(sl0, n, ("f",), first, ntr)["f"]
    assert_bitwise(AM.canon(to_host(t).reshape(want.shape, order="F")), AM.canon(want), f"{s.name} step {s.i}: export of block {sl0, n}")


def nonneg(s, sl0, n, first, ntr):
    """(no draw) sum and nneg NaN-filled between patterned bands, each absent on one call of three"""
    import torch
    sh = s.M.nonneg_shapes(n, s.nx, s.nz, ntr)
    outs = (("sum", "nneg"), ("sum",), ("nneg",))[s.count[s.op] % 3]
    bufs = {k: H.nan_out(sh[k], s.dt) for k in outs}
    kinds = NM.kinds(s.m.a["f"][sl0:sl0 + n, ..., first:first + ntr])
    for k in (NM.KEEP, NM.FIX, NM.ZERO):
        s.rows[k] += int(np.sum(kinds == k))
    torch.cuda.synchronize()
    assert s.code(s.p.nonneg, bufs["sum"][2] if "sum" in bufs else None, bufs["nneg"][2] if "nneg" in bufs else None, sl0, n, first,
                  ntr) is None
    s.p.sync()
    want = dict(zip(("sum", "nneg"), s.m.nonneg(sl0=sl0, n=n, first=first, ntr=ntr)))
    for k, (raw, pristine, view) in bufs.items():
        assert H.bands_kept(raw, pristine)
        assert_bitwise(to_host(view), want[k], s.at(k, sl0, n, first, ntr))


def nonneg_refused(s, sl0, n, first, ntr):
    M, ncrms, T = s.M, s.ncrms, s.T
    bad = [(ncrms, 1, 0, 1), (0, 1, T, 1), (0, 1, 0, T + 1), (-1, 1, 0, 1)][s.count[s.op] % 4]
    got = s.code(s.p.nonneg, None, None, *bad)
    assert got == M.EINVAL == s.m.nonneg(sl0=bad[0], n=bad[1], first=bad[2], ntr=bad[3])


def relax(s, sl0, n, first, ntr):
    """the plain form of relax to the horizontal mean"""
    c = RM.make_c(n, s.nz, s.dt, s.seed_of_step())
    assert s.code(s.p.relax, to_dev(c), None, None, sl0, n, first, ntr) is None
    assert not isinstance(s.m.relax(c, None, sl0=sl0, n=n, first=first, ntr=ntr), int)


@pytest.mark.parametrize("name,shape,T,dt,sw,seed", CASES, ids=[c[0] for c in CASES])
def test_sequence_with_nonneg(mpdata, oracle, name, shape, T, dt, sw, seed):
    # (no case asks for the reference layout)
    s = Sequence(mpdata, oracle, Model, NM.make_plan_inputs, name, (shape, T, dt, sw), seed, ref=False,
                   windows=bool(sw.get("tall")), periodic=bool(sw.get("periodic")))
    s.rows = {NM.KEEP: 0, NM.FIX: 0, NM.ZERO: 0}
    # (a windowed plan: nonneg behind the import, behind a run, behind a nonneg, and in front of a sediment and a subside,
    # which refresh the seams it marked stale; a periodic one: stale halos, then a run and a block export right behind
    # the call)
    count = s.play(["nonneg", "run", "level_add", "nonneg", "sediment", "nonneg", "subside", "nonneg", "relax", "nonneg",
                    "set_boundary", "run_tracers", "cell_add", "nonneg", "export_block", "import_block", "nonneg", "run", "nonneg",
                    "export", "import", "nonneg", "nonneg", "run", "nonneg_refused", "nonneg"], OPS, STEPS,
                   {"nonneg": nonneg, "nonneg_refused": nonneg_refused, "relax": relax, "cell_add": H.plain_cell_add(0.75), "export": export,
                    "export_block": export_block})
    assert count["nonneg"] >= 10 and count["run"] + count["run_tracers"] >= 4
    assert count["subside"] >= 1 and count["sediment"] >= 1 and count["relax"] >= 1 and count["level_add"] >= 1
    assert count["cell_add"] >= 1 and count["import"] >= 1 and count["import_block"] >= 1 and count["nonneg_refused"] >= 1
    assert min(s.rows.values()) > 0, s.rows                  # the calls met rows of every kind
