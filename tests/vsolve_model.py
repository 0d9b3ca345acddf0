"""The model of the implicit vertical solve (include/mpdata_hip.h 3o) in plain numpy, the inputs its tests share, and the
plan model with the new call.

factor(lo, di, up): (n, nzm) each -> (p, g) (n, nzm).  vsolve(f, lo, di, up): the arrays of ONE block in the reference
layout -- f (n, nx+6, nzm[, T]) -- -> f_new.  Every statement below is one elementwise operation on arrays of f's dtype,
hence one rounding per element, in the definition's order: the factors per (instance, level), the forward sweep y and the
backward sweep x per (instance, column, tracer).  Every f on the right is the old one.  Only the interior columns 1 .. nx
(array index 3 .. nx+2) of f_new differ from f; halo columns are not read.  lo[:, 0] and up[:, nzm-1] are not read.
"""
import numpy as np

from oracle.plan_model import EINVAL, ESTATE, EUNSUPPORTED, PlanModel
from util import bits


def factor(lo, di, up):
    lo, di, up = np.asarray(lo), np.asarray(di), np.asarray(up)
    dt = di.dtype
    n, nzm = di.shape
    assert lo.dtype == dt and up.dtype == dt and lo.shape == di.shape == up.shape, (lo.dtype, up.dtype, lo.shape, up.shape)
    one = dt.type(1)
    p, g = np.zeros((n, nzm), dt), np.zeros((n, nzm), dt)
    p[:, 0] = one / di[:, 0]
    if nzm > 1:
        g[:, 0] = up[:, 0] * p[:, 0]
    for k in range(1, nzm):
        m = lo[:, k] * g[:, k - 1]
        d = di[:, k] - m
        p[:, k] = one / d
        if k + 1 < nzm:
            g[:, k] = up[:, k] * p[:, k]                    # (g of the top level is not used)
        assert m.dtype == dt and d.dtype == dt
    assert p.dtype == dt and g.dtype == dt
    return p, g


def forward(c, lo, p, y_prev=None, k_first=0):
    """the forward sweep on the levels of c (n, nx, m, T) that stand for the levels k_first .. of lo, p (n, m): y_prev
    (n, nx, T) the carry from the level below, None at the bottom of the column -> (y, carry)"""
    dt = c.dtype
    y = np.empty_like(c)
    for k in range(c.shape[2]):
        if y_prev is None:
            assert k == 0 and k_first == 0
            y[:, :, k] = c[:, :, k] * p[:, None, k, None]
        else:
            m = lo[:, None, k, None] * y_prev
            r = c[:, :, k] - m
            y[:, :, k] = r * p[:, None, k, None]
            assert m.dtype == dt and r.dtype == dt
        y_prev = y[:, :, k]
    assert y.dtype == dt
    return y, y_prev


def backward(y, g, x_next=None):
    """the backward sweep on the levels of y (n, nx, m, T) with g (n, m): x_next (n, nx, T) the carry from the level above,
    None at the top of the column -> (x, carry)"""
    dt = y.dtype
    x = np.empty_like(y)
    for k in range(y.shape[2] - 1, -1, -1):
        if x_next is None:
            x[:, :, k] = y[:, :, k]
        else:
            m = g[:, None, k, None] * x_next
            x[:, :, k] = y[:, :, k] - m
            assert m.dtype == dt
        x_next = x[:, :, k]
    assert x.dtype == dt
    return x, x_next


def vsolve(f, lo, di, up):
    f = np.asarray(f)
    dt = f.dtype
    one_tracer = f.ndim == 3
    F = f.reshape(f.shape + (1,)) if one_tracer else f
    n, nxp6, nzm, T = F.shape
    nx = nxp6 - 6
    for a in (lo, di, up):
        assert np.asarray(a).dtype == dt and np.asarray(a).shape == (n, nzm), (np.asarray(a).dtype, np.asarray(a).shape, (n, nzm))
    p, g = factor(lo, di, up)
    ci = F[:, 3:nx + 3]                                     # columns 1 .. nx
    y, _ = forward(ci, np.asarray(lo), p)
    x, _ = backward(y, g)
    out = np.array(F, order="F")
    out[:, 3:nx + 3] = x
    assert out.dtype == dt
    return np.asfortranarray(out[..., 0] if one_tracer else out)


# ---- inputs.  lo, up uniform in [-0.4, 0), di = 1 - lo - up (formed in float64, then rounded to the dtype): strictly diagonally dominant by rows with
# |di| - |lo| - |up| = 1, so the inverse has infinity norm <= 1 and max|x| <= max|f| up to rounding: chains of calls and
# runs stay finite.
def make_coeffs(n, nz, dtype=np.float64, seed=0):
    """(lo, di, up) (n, nzm) of a block of n instances, Fortran order"""
    rng = np.random.default_rng([seed, n, nz, 3])
    lo = np.asfortranarray(rng.uniform(-0.4, 0.0, (n, nz - 1)).astype(dtype))
    up = np.asfortranarray(rng.uniform(-0.4, 0.0, (n, nz - 1)).astype(dtype))
    one = np.dtype(dtype).type(1)
    di = np.asfortranarray((one.astype(np.float64) - lo.astype(np.float64) - up.astype(np.float64)).astype(dtype))
    assert lo.dtype == di.dtype == up.dtype == np.dtype(dtype)
    return lo, di, up


def make_plan_inputs(oracle, shape, T=1, dtype=np.float64, seed=100):
    """the seven arrays of a plan, as subside_model.make_plan_inputs makes them: f signed, in [-0.5, 0.5); rho and adz
    in [0.5, 1); f and flux carry a tracer axis only for T > 1"""
    import subside_model
    return subside_model.make_plan_inputs(oracle, shape, T, dtype, seed)


class PlanModelVsolve(PlanModel):
    """oracle.plan_model.PlanModel with section 3o.  The block rule: only instances [sl0, sl0 + n) and tracers [first,
    first + ntr) change.  The error order: the block, the handle, the range, the tracers, the NULLs, the precision of a
    host form, the state.  The interior-only rule: halo columns are neither read nor written.  The periodic rule: no wrap
    is part of the call; the halos a PERIODIC model then holds are those of the OLD field, and every read-back and run of
    the model wraps again, as the plan does after the call cleared its marks.  Windows, seams and the phantom have no
    face here: a windowed plan must hold what the tall model holds."""
    multi = False

    def vsolve(self, lo, di, up, sl0=0, n=None, first=0, ntr=None, eb=None):
        """-> None, or the code"""
        ncrms, nx, nz, T = self.dims
        n = ncrms - sl0 if n is None else n
        ntr = T - first if ntr is None else ntr
        if n < 1 or sl0 < 0:
            return EINVAL
        if self.multi:
            return EUNSUPPORTED
        if sl0 + n > ncrms or not self._tracers_ok(first, ntr):
            return EINVAL
        if lo is None or di is None or up is None:
            return EINVAL
        if eb is not None and eb != np.dtype(self.dtype).itemsize:
            return ESTATE
        if not self.uploaded:
            return ESTATE
        blk = self.a["f"][sl0:sl0 + n, ..., first:first + ntr]
        self.a["f"][sl0:sl0 + n, ..., first:first + ntr] = vsolve(blk, lo, di, up)
        self._note()
        return None
