"""The model of the per-cell sources (include/mpdata_hip.h 3p) in plain numpy, the inputs its tests share, and the plan
model with the new call.

cell_add(f, s, c, mode): the arrays of ONE block in the reference layout -- f (n, nx+6, nzm[, T]), s (n, nx, nzm[, T]) --
-> (f_new, dsum (n, nzm[, T])).  Every statement below is one elementwise operation on arrays of f's dtype, hence one
rounding per element, in the definition's association: the factor c rounded once to f's dtype, the product p = c * s, the
sum g = f + p, under CLIP the maximum with zero, the difference g - f_old; the sum of dsum is an explicit loop over i = 1
.. nx from +0.  Only the interior columns 1 .. nx (array index 3 .. nx+2) of f_new differ from f; halo columns are not read.
"""
import numpy as np

from oracle.plan_model import EINVAL, ESTATE, EUNSUPPORTED, PlanModel
from util import bits

ADD, CLIP = 0, 1


def cell_add(f, s, c=1.0, mode=ADD):
    f = np.asarray(f)
    dt = f.dtype
    one_tracer = f.ndim == 3
    F = f.reshape(f.shape + (1,)) if one_tracer else f
    n, nxp6, nzm, T = F.shape
    nx = nxp6 - 6
    s = np.asarray(s)
    S = s.reshape(s.shape + (1,)) if s.ndim == 3 else s
    assert S.dtype == dt and S.shape == (n, nx, nzm, T), (S.dtype, S.shape, (n, nx, nzm, T))
    assert mode in (ADD, CLIP)
    cf = dt.type(c)                                         # the one rounding of the factor
    ci = F[:, 3:nx + 3]                                     # columns 1 .. nx
    p = cf * S
    g = ci + p
    if mode == CLIP:
        g = np.maximum(dt.type(0), g)
    d = g - ci
    out = np.array(F, order="F")
    out[:, 3:nx + 3] = g
    dsum = np.zeros((n, nzm, T), dt)                        # +0
    for i in range(nx):
        dsum = dsum + d[:, i]
    for x in (p, g, d, out, dsum):
        assert x.dtype == dt
    if one_tracer:
        out, dsum = out[..., 0], dsum[..., 0]
    return np.asfortranarray(out), np.asfortranarray(dsum)


def clipped_fraction(f, s, c):
    """the share of the interior cells of the block on which CLIP acts (f + c * s < 0)"""
    f = np.asarray(f)
    F = f.reshape(f.shape + (1,)) if f.ndim == 3 else f
    S = np.asarray(s)
    S = S.reshape(S.shape + (1,)) if S.ndim == 3 else S
    g = F[:, 3:F.shape[1] - 3] + F.dtype.type(c) * S
    return float(np.mean(g < 0))


# ---- inputs.  s: uniform in [-0.5, 0.5), another value per cell and tracer.  With |c| <= 1 a call adds at most a half
# to |f|: a chain of a few calls and runs stays finite.
def make_s(n, nx, nz, T=None, dtype=np.float64, seed=0):
    """s (n, nx, nzm[, T]) of a block of n instances, Fortran order; T None: one tracer without the axis"""
    rng = np.random.default_rng([seed, n, nx, nz, 0 if T is None else T])
    sh = (n, nx, nz - 1) + (() if T is None else (T,))
    return np.asfortranarray(rng.uniform(-0.5, 0.5, sh).astype(dtype))


def make_plan_inputs(oracle, shape, T=1, dtype=np.float64, seed=100):
    """the seven arrays of a plan, as subside_model.make_plan_inputs makes them: f signed, in [-0.5, 0.5); rho and adz
    in [0.5, 1); f and flux carry a tracer axis only for T > 1"""
    import subside_model
    return subside_model.make_plan_inputs(oracle, shape, T, dtype, seed)


class PlanModelCellAdd(PlanModel):
    """oracle.plan_model.PlanModel with section 3p.  The block rule: only instances [sl0, sl0 + n) and tracers [first,
    first + ntr) change.  The error order: the block, the handle, the range, the tracers, the NULL, the mode, the
    precision of a host form, the state.  The interior-only rule: halo columns are neither read nor written.  The
    periodic rule: no wrap is part of the call and the plan clears its halo marks; the halos a PERIODIC model then holds
    are those of the OLD field, and every read-back and run of the model wraps again, as the plan does with cleared
    marks.  The windowed rule (the scheme 3p chose): the plan writes owned levels only and clears the seam marks of the
    range, so its next run refreshes every other copy from the owners; the model holds the tall column, which is what the
    owners hold, so a windowed plan must give the model's bits after the call and after the run behind it, whether its
    seams were fresh or stale at the call.  Seams and the phantom have no other face here."""
    multi = False

    def cell_add(self, s, c=1.0, mode=ADD, sl0=0, n=None, first=0, ntr=None, eb=None):
        """-> dsum with a tracer axis, or the code"""
        ncrms, nx, nz, T = self.dims
        n = ncrms - sl0 if n is None else n
        ntr = T - first if ntr is None else ntr
        if n < 1 or sl0 < 0:
            return EINVAL
        if self.multi:
            return EUNSUPPORTED
        if sl0 + n > ncrms or not self._tracers_ok(first, ntr):
            return EINVAL
        if s is None:
            return EINVAL
        if mode not in (ADD, CLIP):
            return EINVAL
        if eb is not None and eb != np.dtype(self.dtype).itemsize:
            return ESTATE
        if not self.uploaded:
            return ESTATE
        s = np.asarray(s)
        s = s.reshape(s.shape + (1,)) if s.ndim == 3 else s
        new, dsum = cell_add(self.a["f"][sl0:sl0 + n, ..., first:first + ntr], s, c, mode)
        self.a["f"][sl0:sl0 + n, ..., first:first + ntr] = new
        self._note()
        return dsum
