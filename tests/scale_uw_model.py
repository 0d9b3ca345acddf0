"""The model of the per-instance velocity scaling (include/mpdata_hip.h 3j) in plain numpy, the factors and inputs its
tests share, and the plan model with the new call.

scale_uw(u, w, su, sw): u (n, nx+5, nzm), w (n, nx+4, nz) in the reference layout, su, sw (n,) of the same dtype or None:
the factor broadcast over the column and level axes in the array's dtype -- one rounded multiply per element, level nz
of w included.  None leaves that array as it is.

Inputs: those of tests/courant_model.py (shapes of tests/level_stats_model.py LM.INPUTS; signed velocities, rho and adz
in [0.5, 1.5)) with u and w multiplied by 2**-4.  The scaling is exact, so every mantissa stays full, and it puts the
outflow Courant number below (1/32 + 1/32 + 2/16) * 2 = 3/8 <= 1/2, where the upwind pass stays non-negative
(tests/test_courant_cpu.py): the step is stable, so the FAST variant's bound of the README (max|df| <= 64 u max|f_in|),
which is stated for stable steps, applies to a run on them.  The factors have magnitude <= 1 and keep it so.
"""
import numpy as np

import courant_model as CM
import level_add_model as AM
import level_stats_model as LM
from oracle.plan_model import EINVAL, ESTATE, EUNSUPPORTED

FACTORS = ((1, 1), (1, 2), (1, 3), (1, 5), (3, 7), (-1, 3), (0, 1))   # 1/3, 1/5 and 3/7 make the product round


def scale_uw(u, w, su=None, sw=None):
    """-> (u * su, w * sw), Fortran order; an array whose factor is None comes back as a copy"""
    out = []
    for a, s in ((u, su), (w, sw)):
        a = np.asarray(a)
        if s is None:
            out.append(np.array(a, order="F"))
            continue
        s = np.asarray(s)
        assert s.dtype == a.dtype and s.shape == a.shape[:1], (s.dtype, a.dtype, s.shape, a.shape)
        r = a * s[:, None, None]
        assert r.dtype == a.dtype
        out.append(np.asfortranarray(r))
    return out[0], out[1]


def make_s(shape, dtype, seed, n=None):
    """n factors (default: one per instance of `shape` = (ncrms, nx, nz)) drawn from FACTORS, rounded once to dtype;
    consecutive factors are distinct, so an index slip shows"""
    ncrms, _, nz = shape
    n = ncrms if n is None else n
    rng = np.random.default_rng([seed, nz, n])
    vals = np.array([np.dtype(dtype).type(p) / np.dtype(dtype).type(q) for p, q in FACTORS], dtype)
    idx = np.empty(n, np.int64)
    for i in range(n):
        k = int(rng.integers(0, len(vals)))
        while i and k == idx[i - 1]:
            k = int(rng.integers(0, len(vals)))
        idx[i] = k
    s = vals[idx]
    assert s.dtype == np.dtype(dtype)
    return s


def make(oracle, name):
    """the seven arrays of LM.INPUTS[name] (see the module text)"""
    shape, T, dt, _ = LM.INPUTS[name]
    inp = CM.make(oracle, name)
    for k in ("u", "w"):
        inp[k] = np.asfortranarray(inp[k] * dt(2.0 ** -4))
        assert inp[k].dtype == dt
    return inp


def other(oracle, name, shift=50):
    """a second set of velocities of the same kind (run_uw, imports)"""
    _, _, dt, _ = LM.INPUTS[name]
    u, w = CM.other(oracle, name, shift)
    return np.asfortranarray(u * dt(2.0 ** -4)), np.asfortranarray(w * dt(2.0 ** -4))


# the seed of the factors every test of tests/test_plan_scale_uw.py applies FIRST to the u, w of make(oracle, name): su
# from SEEDS[name], sw from SEEDS[name] + 1000 (later ones: + 1, + 2, ...); the seeds are those that pass the guard of
# tests/test_scale_uw_cpu.py -- a seed that misses a condition is replaced here, the conditions stay
SEEDS = {name: 400 for name in LM.INPUTS}
SEEDS.update({"f32-nz28-odd": 401, "f64-blocks": 401, "f32-blocks": 401})   # (400: an instance whose cinst keeps its bits)


def s_like(name, k=0, sl0=0, n=None):
    """(su, sw): the k-th factors of a test on LM.INPUTS[name] (k = 0: the guarded ones), entries sl0 .. sl0+n of the
    whole plan's"""
    shape, _, dt, _ = LM.INPUTS[name]
    n = shape[0] - sl0 if n is None else n
    su, sw = make_s(shape, dt, SEEDS[name] + k), make_s(shape, dt, SEEDS[name] + 1000 + k)
    return np.ascontiguousarray(su[sl0:sl0 + n]), np.ascontiguousarray(sw[sl0:sl0 + n])


class PlanModelScale(AM.PlanModelAdd):
    """oracle.plan_model.PlanModel (with section 3i, tests/level_add_model.py) with section 3j; `multi`: the handle of a
    multi-GPU plan.  The order of the checks is the header's: the range, the NULLs, the state."""

    def scale_uw(self, su=None, sw=None, sl0=0, n=None):
        ncrms = self.dims[0]
        n = ncrms - sl0 if n is None else n
        if n < 1 or sl0 < 0:
            return EINVAL
        if self.multi:
            return EUNSUPPORTED
        if sl0 + n > ncrms:
            return EINVAL
        if su is None and sw is None:
            return EINVAL
        if not self.uploaded:
            return ESTATE
        if (su is not None and not self.have_u) or (sw is not None and not self.have_w):
            return ESTATE
        u, w = scale_uw(self.a["u"][sl0:sl0 + n], self.a["w"][sl0:sl0 + n],
                        None if su is None else np.asarray(su).reshape(n), None if sw is None else np.asarray(sw).reshape(n))
        self.a["u"][sl0:sl0 + n] = u
        self.a["w"][sl0:sl0 + n] = w
        return None
