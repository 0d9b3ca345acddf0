"""The model of the mass-weighted column integrals (include/mpdata_hip.h 3k) in plain numpy, the wrong orders its input
guard measures against, and the plan model with the new call.

column_path(f, rho, adz): f (n, nx+6, nzm[, T]) in the reference layout, rho, adz (n, nzm) of the same dtype.  Per
instance, interior column i = 1 .. nx (array index i + 2) and tracer:
  wgt  = rho * adz                          formed first, rounded to the dtype
  path : s = +0.0; for k = 1 .. nzm:  s = s + wgt_k * f_k     the product rounded to the dtype, then the add -- an explicit
                                                              loop over k with the running sum held in the array dtype
  mass : s = +0.0; for i = 1 .. nx:   s = s + path_i          an explicit loop over i, never np.sum
-> path (n, nx[, T]), mass (n[, T]), Fortran order.

Inputs: LM.INPUTS (and GROUP_INPUTS below) / LM.make of tests/level_stats_model.py (raw magnitudes, columns scaled by 2**-(column mod 4)); the rho
and adz are the ones LM.make returns.  tests/test_column_path_cpu.py checks that they are sharp: the sum in the reversed
order, an fma-contracted sum and a pairwise mass all differ in bits from the defined ones.
"""
from fractions import Fraction

import numpy as np

import level_stats_model as LM
import scale_uw_model as SM
from oracle.plan_model import EINVAL, ESTATE, EUNSUPPORTED


def _weights(f, rho, adz):
    f, rho, adz = np.asarray(f), np.asarray(rho), np.asarray(adz)
    assert rho.dtype == adz.dtype == f.dtype and rho.shape == adz.shape == (f.shape[0], f.shape[2]), (rho.shape, f.shape)
    w = rho * adz
    assert w.dtype == f.dtype
    return f, w.reshape(w.shape + (1,) * (f.ndim - 3))     # (n, nzm[, 1]): broadcasts over the tracers


def mass_of(path):
    """the sequential sum of path (n, nx[, T]) over its columns"""
    path = np.asarray(path)
    m = np.zeros(path.shape[:1] + path.shape[2:], path.dtype)     # +0.0
    for i in range(path.shape[1]):
        m = m + path[:, i]
    assert m.dtype == path.dtype
    return np.asfortranarray(m)


def column_path(f, rho, adz, order=None):
    """-> (path, mass); order: the levels' order of the sum (default: rising)"""
    f, w = _weights(f, rho, adz)
    nx, nzm = f.shape[1] - 6, f.shape[2]
    assert nx >= 1 and nzm >= 1
    s = np.zeros((f.shape[0], nx) + f.shape[3:], f.dtype)          # +0.0
    for k in (range(nzm) if order is None else order):
        prod = w[:, None, k] * f[:, 3:nx + 3, k]                   # rounded to the dtype
        assert prod.dtype == f.dtype
        s = s + prod
    assert s.dtype == f.dtype
    return np.asfortranarray(s), mass_of(s)


def path_reversed(f, rho, adz):
    return column_path(f, rho, adz, order=range(np.asarray(f).shape[2] - 1, -1, -1))[0]


def path_fma_column(f, rho, adz, sl, i, t=None):
    """one column of path with s = fma(wgt_k, f_k, s): the product exact, one rounding per level (rationals, rounded to
    the dtype by numpy's correctly rounding conversion)"""
    f, w = _weights(f, rho, adz)
    col = f[sl, i + 2, :] if t is None else f[sl, i + 2, :, t]
    dt = f.dtype.type
    s = dt(0)
    for k in range(f.shape[2]):
        exact = Fraction(float(s)) + Fraction(float(w[sl, k].reshape(-1)[0])) * Fraction(float(col[k]))
        # a rational -> the nearest real of the dtype: Python's correctly rounded integer division (fp64), _round_f32
        s = dt(exact.numerator / exact.denominator) if f.dtype == np.float64 else dt(_round_f32(exact))
    return s


def _round_f32(x):
    """the fp32 nearest (ties to even) to the rational x"""
    if x == 0:
        return np.float32(0)
    lo = np.float32(float(x))                       # a candidate: within one ulp
    best = lo
    for c in (np.nextafter(lo, np.float32(-np.inf)), np.nextafter(lo, np.float32(np.inf))):
        d_c, d_b = abs(Fraction(float(c)) - x), abs(Fraction(float(best)) - x)
        if d_c < d_b or (d_c == d_b and not (int(np.float32(c).view(np.uint32)) & 1)):
            best = c
    return np.float32(best)


def mass_pairwise(path):
    """the tree sum ((p1 + p2) + (p3 + p4)) + ... of path over its columns"""
    path = np.asarray(path)
    parts = [np.array(path[:, i]) for i in range(path.shape[1])]
    while len(parts) > 1:
        parts = [parts[j] + parts[j + 1] if j + 1 < len(parts) else parts[j] for j in range(0, len(parts), 2)]
    return parts[0]


# Inputs of more than one workgroup GROUP of the plan-layout kernel (csrc/mpdata_column_path.hip: a workgroup takes UG
# adjacent 8-byte elements of the instance axis -- 16; 32 at nz <= 8; an fp32 element is a pair of instances): the plans of
# LM.INPUTS all fit one group.  name -> (shape, tracers, dtype, seed) as LM.INPUTS, and GROUP_REALS[name] = instances per group.
GROUP_INPUTS = {
    "f64-g40-nz28": ((40, 7, 28), 1, LM.F64, 100),          # 16 + 16 + 8 instances: three groups, the last one partly padding
    "f32-g41-nz28-odd": ((41, 7, 28), 1, LM.F32, 100),      # 21 pairs, the last one half phantom: two groups
    "f64-g70-nz5": ((70, 7, 5), 2, LM.F64, 100),            # UG = 32, 8 instances per tile: three groups, two tracers
    "f64-g20-nz72": ((20, 7, 72), 1, LM.F64, 100),          # one-instance tiles of two slices: two groups
    "f64-g20-tall": ((20, 7, 250), 1, LM.F64, 100),         # windows: two groups of instances, five tiles each
    "f32-g37-tall-odd": ((37, 7, 250), 1, LM.F32, 100),     # windows, pairs, phantom: two groups
}
GROUP_REALS = {"f64-g40-nz28": 16, "f32-g41-nz28-odd": 32, "f64-g70-nz5": 32, "f64-g20-nz72": 16, "f64-g20-tall": 16,
               "f32-g37-tall-odd": 32}
INPUTS = dict(LM.INPUTS, **GROUP_INPUTS)


def group_blocks(name):
    """(sl0, n) blocks of GROUP_INPUTS[name]: one that starts inside the second group (the launch's first group is not group
    0), one that straddles the boundary of the first two groups, one that ends inside the first group, one from the boundary to
    the end of the plan"""
    ncrms, B = GROUP_INPUTS[name][0][0], GROUP_REALS[name]
    assert ncrms > B + 3
    return ((B + 1, 3), (B - 3, 6), (1, B - 4), (B, ncrms - B))


# the seeds of the inputs: those of INPUTS where they pass the guard of tests/test_column_path_cpu.py -- a seed that
# misses a condition is replaced here, the conditions stay (the three below: a mass whose tree sum has the defined bits)
SEEDS = {name: v[3] for name, v in INPUTS.items()}
SEEDS.update({"f64-nz130": 101, "f64-nx5": 102, "f32-tall-odd": 101})


def make(oracle, name, shift=0):
    """the seven arrays of INPUTS[name] from SEEDS[name] + shift (shift != 0: a second set, for run_uw and imports)"""
    shape, T, dt, _ = INPUTS[name]
    return LM.make(oracle, shape, T, dt, SEEDS[name] + shift)


class PlanModelPath(SM.PlanModelScale):
    """oracle.plan_model.PlanModel (with sections 3i and 3j) with section 3k: the call changes nothing, so the model's is a
    no-op that returns the code the header promises -- the range, the tracers, the NULL, the state, in 3g's order"""

    def column_path(self, sl0=0, n=None, first=0, ntr=None, path=True):
        ncrms = self.dims[0]
        n = ncrms - sl0 if n is None else n
        ntr = self.dims[3] - first if ntr is None else ntr
        if n < 1 or sl0 < 0:
            return EINVAL
        if self.multi:
            return EUNSUPPORTED
        if sl0 + n > ncrms:
            return EINVAL
        if not self._tracers_ok(first, ntr) or not path:
            return EINVAL
        if not self.uploaded:
            return ESTATE
        return None

    def paths(self, sl0=0, n=None, first=0, ntr=None):
        """(path (n, nx, ntr), mass (n, ntr)) of what the model holds now"""
        ncrms = self.dims[0]
        n = ncrms - sl0 if n is None else n
        ntr = self.dims[3] - first if ntr is None else ntr
        b = slice(sl0, sl0 + n)
        return column_path(self.a["f"][b, ..., first:first + ntr], self.a["rho"][b], self.a["adz"][b])
