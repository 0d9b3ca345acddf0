"""The model of the relaxation to a level profile (include/mpdata_hip.h 3r) in plain numpy, the inputs its tests share,
and the plan model with the new call.

relax(f, c, target): the arrays of ONE block in the reference layout -- f (n, nx+6, nzm[, T]), c (n, nzm), target (n,
nzm[, T]) or None -- -> (f_new, mean (n, nzm[, T])).  Every statement below is one elementwise operation on arrays of f's
dtype, hence one rounding per element, in the definition's association: without a target the sum is an explicit loop over
i = 1 .. nx from +0 and m = s / nx ONE numpy division by nx in f's dtype (numpy's division is the IEEE one); then d = f - m,
p = c * d, g = f - p.  Levels with c == 0 (either sign) are copied, not computed.  Only the interior columns 1 .. nx (array
index 3 .. nx+2) of f_new differ from f; halo columns are not read.
"""
import numpy as np

from oracle.plan_model import EINVAL, ESTATE, EUNSUPPORTED, PlanModel
from util import bits


def relax(f, c, target=None):
    f = np.asarray(f)
    dt = f.dtype
    one_tracer = f.ndim == 3
    F = f.reshape(f.shape + (1,)) if one_tracer else f
    n, nxp6, nzm, T = F.shape
    nx = nxp6 - 6
    c = np.asarray(c)
    assert c.dtype == dt and c.shape == (n, nzm), (c.dtype, c.shape, (n, nzm))
    ci = F[:, 3:nx + 3]                                     # columns 1 .. nx
    if target is None:
        s = np.zeros((n, nzm, T), dt)                       # +0
        for i in range(nx):
            s = s + ci[:, i]
        m = s / dt.type(nx)                                 # nx is exact in either precision; one rounded division
    else:
        t = np.asarray(target)
        m = np.array(t.reshape(t.shape + (1,)) if t.ndim == 2 else t)
        assert m.dtype == dt and m.shape == (n, nzm, T), (m.dtype, m.shape, (n, nzm, T))
    d = ci - m[:, None]
    p = c[:, None, :, None] * d
    g = ci - p
    for x in (m, d, p, g):
        assert x.dtype == dt
    out = np.array(F, order="F")
    out[:, 3:nx + 3] = np.where((c != 0)[:, None, :, None], g, ci)   # c == 0: the level keeps every bit
    if one_tracer:
        out, m = out[..., 0], m[..., 0]
    return np.asfortranarray(out), np.asfortranarray(m)


def changed_fraction(f, c, target=None, sl0=0, n=None, first=0, ntr=None):
    """the share of the interior cells of the block and the tracer range that a call changes (bitwise)"""
    f = np.asarray(f)
    F = f.reshape(f.shape + (1,)) if f.ndim == 3 else f
    n = F.shape[0] - sl0 if n is None else n
    ntr = F.shape[3] - first if ntr is None else ntr
    blk = np.asfortranarray(F[sl0:sl0 + n, ..., first:first + ntr])
    new, _ = relax(blk, c, target)
    nx = F.shape[1] - 6
    return float(np.mean(bits(new[:, 3:nx + 3]) != bits(blk[:, 3:nx + 3])))


# ---- inputs.  c: zero on the lower half of the levels, uniform in (0, 1] above -- the shape of a damping layer; every
# instance has its own values.  target: uniform in [-0.5, 0.5).  With 0 <= c <= 1 a call moves f towards m: a chain of
# calls and runs stays bounded by what it started from.
def make_c(n, nz, dtype=np.float64, seed=0):
    """c (n, nzm), Fortran order"""
    rng = np.random.default_rng([seed, n, nz, 1])
    nzm = nz - 1
    c = 1.0 - rng.uniform(0.0, 1.0, (n, nzm))               # (0, 1]
    c[:, :nzm // 2] = 0.0
    c = c.astype(dtype)
    c[:, nzm // 2:][c[:, nzm // 2:] == 0] = 1               # (a value that rounded to zero in fp32)
    return np.asfortranarray(c)


def make_target(n, nz, T=None, dtype=np.float64, seed=0):
    """target (n, nzm[, T]) of a block of n instances, Fortran order; T None: one tracer without the axis"""
    rng = np.random.default_rng([seed, n, nz, 0 if T is None else T, 2])
    sh = (n, nz - 1) + (() if T is None else (T,))
    return np.asfortranarray(rng.uniform(-0.5, 0.5, sh).astype(dtype))


def make_plan_inputs(oracle, shape, T=1, dtype=np.float64, seed=100):
    """the seven arrays of a plan, as subside_model.make_plan_inputs makes them: f signed, in [-0.5, 0.5); rho and adz
    in [0.5, 1); f and flux carry a tracer axis only for T > 1"""
    import subside_model
    return subside_model.make_plan_inputs(oracle, shape, T, dtype, seed)


class PlanModelRelax(PlanModel):
    """oracle.plan_model.PlanModel with section 3r.  The block rule: only instances [sl0, sl0 + n) and tracers [first,
    first + ntr) change.  The error order: the block, the handle, the range, the tracers, the NULL c, the precision of a
    host form, the state.  The interior-only rule: halo columns are neither read nor written -- the mean is that of the
    interior.  The periodic rule: no wrap is part of the call and the plan clears its halo marks; the halos a PERIODIC
    model then holds are those of the OLD field, and every read-back and run of the model wraps again, as the plan does
    with cleared marks.  The windowed rule (the scheme 3r chose, that of 3p): the plan reads and writes owned levels only
    and clears the seam marks of the range, so its next run refreshes every other copy from the owners; the model holds
    the tall column, which is what the owners hold, so a windowed plan must give the model's bits after the call and
    after the run behind it, whether its seams were fresh or stale at the call."""
    multi = False

    def relax(self, c, target=None, sl0=0, n=None, first=0, ntr=None, eb=None):
        """-> mean with a tracer axis, or the code"""
        ncrms, nx, nz, T = self.dims
        n = ncrms - sl0 if n is None else n
        ntr = T - first if ntr is None else ntr
        if n < 1 or sl0 < 0:
            return EINVAL
        if self.multi:
            return EUNSUPPORTED
        if sl0 + n > ncrms or not self._tracers_ok(first, ntr):
            return EINVAL
        if c is None:
            return EINVAL
        if eb is not None and eb != np.dtype(self.dtype).itemsize:
            return ESTATE
        if not self.uploaded:
            return ESTATE
        if target is not None:
            target = np.asarray(target)
            target = target.reshape(target.shape + (1,)) if target.ndim == 2 else target
        new, mean = relax(self.a["f"][sl0:sl0 + n, ..., first:first + ntr], c, target)
        self.a["f"][sl0:sl0 + n, ..., first:first + ntr] = new
        self._note()
        return mean
