"""The model of the per-level increments (include/mpdata_hip.h 3i) in plain numpy, the increments its tests share, and
the plan model with the new call.

level_add(f, d, clip): f (n, nx+6, nzm[, T]) in the reference layout, d (n, nzm[, T]): d broadcast over the column axis
(every column, halos included) in f's dtype -- one rounded add per element --, then max(0, .) for MPDATA_LEVEL_ADD_CLIP.
The shapes and the f of the tests are those of tests/level_stats_model.py (LM.INPUTS, LM.make): f there lies in (0, 1],
so a d drawn from (-1, 1) is signed, of f's magnitude range, and makes f + d negative on part of the cells.
"""
import numpy as np

import level_stats_model as LM
from oracle.plan_model import EINVAL, ESTATE, EUNSUPPORTED, PlanModel

ADD, CLIP = 0, 1            # MPDATA_LEVEL_ADD, MPDATA_LEVEL_ADD_CLIP


def level_add(f, d, clip=False):
    f, d = np.asarray(f), np.asarray(d)
    assert d.dtype == f.dtype and d.shape == f.shape[:1] + f.shape[2:], (d.dtype, f.dtype, d.shape, f.shape)
    out = f + d[:, None]
    out = np.maximum(f.dtype.type(0), out) if clip else out
    assert out.dtype == f.dtype
    return np.asfortranarray(out)


def canon(a):
    """-0.0 -> +0.0 (the sign of a zero result of CLIP is unspecified)"""
    a = np.array(a, order="F")
    a[a == 0] = 0
    return a


def make_d(shape, T, dtype, seed, n=None):
    """d (n, nzm[, T]) for a problem of `shape` = (ncrms, nx, nz): signed, in (-1, 1), Fortran order; n: the instances
    (default: all of the plan's)"""
    ncrms, _, nz = shape
    n = ncrms if n is None else n
    rng = np.random.default_rng([seed, nz, T, n])
    sh = (n, nz - 1) + ((T,) if T > 1 else ())
    # a product (a full mantissa at every size) over four binades, as f's columns are scaled (LM.make)
    d = (rng.uniform(-1.0, 1.0, sh) * rng.uniform(0.5, 1.0, sh) * 2.0 ** -rng.integers(0, 4, sh)).astype(dtype)
    return np.asfortranarray(d)


# the seed of the d every test of tests/test_plan_level_add.py adds FIRST to the f of LM.INPUTS[name] (the later ones
# are SEED + 1, + 2, ... on fields no guard covers); the seeds are those that pass the guard of
# tests/test_level_add_cpu.py -- a seed that misses a condition is replaced here, the conditions stay
SEEDS = {name: 300 for name in LM.INPUTS}


def first_d(name, n=None):
    shape, T, dt, _ = LM.INPUTS[name]
    return make_d(shape, T, dt, SEEDS[name], n)


class PlanModelAdd(PlanModel):
    """oracle.plan_model.PlanModel with section 3i; `multi`: the handle of a multi-GPU plan"""
    multi = False

    def level_add(self, d, sl0=0, n=None, mode=ADD, first=0):
        ncrms, _, nz, _ = self.dims
        n = ncrms - sl0 if n is None else n
        if n < 1 or sl0 < 0:
            return EINVAL
        if self.multi:
            return EUNSUPPORTED
        if sl0 + n > ncrms:
            return EINVAL
        ntr = 1 if d is None or np.ndim(d) < 3 else np.shape(d)[2]
        if not self._tracers_ok(first, ntr) or d is None or mode not in (ADD, CLIP):
            return EINVAL
        if not self.uploaded:
            return ESTATE
        d = np.asarray(d).reshape((n, nz - 1, ntr), order="F")
        self.a["f"][sl0:sl0 + n, ..., first:first + ntr] = level_add(self.a["f"][sl0:sl0 + n, ..., first:first + ntr], d, mode == CLIP)
        self._note()
        return None
