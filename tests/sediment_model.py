"""The model of the sedimentation (include/mpdata_hip.h 3n) in plain numpy, the inputs its tests share, and the plan model
with the new call.

sediment(f, rho, adz, wp): the arrays of ONE block in the reference layout -- f (n, nx+6, nzm[, T]), rho, adz (n, nzm), wp
(n, nx, nzm[, T]) -- -> (f_new, psfc (n, nx[, T]), pflux (n, nzm[, T])).  Every statement below is one elementwise
operation on arrays of f's dtype, hence one rounding per element, in the definition's association: the product Fz, the
product rho * adz, the IEEE quotient, the difference of the two fluxes, its product with the quotient, the final
subtraction; the sum of pflux is an explicit loop over i = 1 .. nx from +0.  Every f on the right is the old one.  Only the
interior columns 1 .. nx (array index 3 .. nx+2) of f_new differ from f; halo columns are not read.
"""
import numpy as np

from oracle.plan_model import EINVAL, ESTATE, EUNSUPPORTED, PlanModel
from util import bits


def sediment(f, rho, adz, wp):
    f = np.asarray(f)
    dt = f.dtype
    one_tracer = f.ndim == 3
    F = f.reshape(f.shape + (1,)) if one_tracer else f
    n, nxp6, nzm, T = F.shape
    nx = nxp6 - 6
    wp = np.asarray(wp)
    Wp = wp.reshape(wp.shape + (1,)) if wp.ndim == 3 else wp
    assert Wp.dtype == dt and Wp.shape == (n, nx, nzm, T), (Wp.dtype, Wp.shape, (n, nx, nzm, T))
    for a in (rho, adz):
        assert np.asarray(a).dtype == dt and np.asarray(a).shape == (n, nzm), (np.asarray(a).dtype, np.asarray(a).shape)
    ci = F[:, 3:nx + 3]                                     # columns 1 .. nx
    fz = np.zeros((n, nx, nzm + 1, T), dt)                  # Fz(i, nz) = +0
    fz[:, :, :nzm] = Wp * ci
    ra = np.asarray(rho) * np.asarray(adz)
    ir = (dt.type(1) / ra)[:, None, :, None]
    d = fz[:, :, :nzm] - fz[:, :, 1:]
    dec = d * ir
    out = np.array(F, order="F")
    out[:, 3:nx + 3] = ci - dec
    psfc = np.array(fz[:, :, 0], order="F")
    pflux = np.zeros((n, nzm, T), dt)                       # +0
    for i in range(nx):
        pflux = pflux + fz[:, i, :nzm]
    for x in (fz, ra, ir, d, dec, out, psfc, pflux):
        assert x.dtype == dt
    if one_tracer:
        out, psfc, pflux = out[..., 0], psfc[..., 0], pflux[..., 0]
    return np.asfortranarray(out), np.asfortranarray(psfc), np.asfortranarray(pflux)


# ---- inputs.  wp: uniform in [-0.05, 0.2), another value per cell and tracer.  With rho, adz in [0.5, 1) the quotient
# is at most 4, so |f_new| <= (1 + 2 * 0.2 * 4) |f|: a chain of a few calls and runs stays finite.
def make_wp(n, nx, nz, T=None, dtype=np.float64, seed=0):
    """wp (n, nx, nzm[, T]) of a block of n instances, Fortran order; T None: one tracer without the axis"""
    rng = np.random.default_rng([seed, n, nx, nz, 0 if T is None else T])
    sh = (n, nx, nz - 1) + (() if T is None else (T,))
    return np.asfortranarray(rng.uniform(-0.05, 0.2, sh).astype(dtype))


def make_plan_inputs(oracle, shape, T=1, dtype=np.float64, seed=100):
    """the seven arrays of a plan, as subside_model.make_plan_inputs makes them: f signed, in [-0.5, 0.5); rho and adz
    in [0.5, 1); f and flux carry a tracer axis only for T > 1"""
    import subside_model
    return subside_model.make_plan_inputs(oracle, shape, T, dtype, seed)


class PlanModelSediment(PlanModel):
    """oracle.plan_model.PlanModel with section 3n.  The block rule: only instances [sl0, sl0 + n) and tracers [first,
    first + ntr) change.  The error order: the block, the handle, the range, the tracers, the NULL, the precision of a
    host form, the state.  The interior-only rule: halo columns are neither read nor written.  The periodic rule: no wrap
    is part of the call; the halos a PERIODIC model then holds are those of the OLD field, and every read-back and run of
    the model wraps again, as the plan does after the call cleared its marks.  Windows, seams and the phantom have no
    face here: a windowed plan must hold what the tall model holds."""
    multi = False

    def sediment(self, wp, sl0=0, n=None, first=0, ntr=None, eb=None):
        """-> (psfc, pflux) with a tracer axis, or the code"""
        ncrms, nx, nz, T = self.dims
        n = ncrms - sl0 if n is None else n
        ntr = T - first if ntr is None else ntr
        if n < 1 or sl0 < 0:
            return EINVAL
        if self.multi:
            return EUNSUPPORTED
        if sl0 + n > ncrms or not self._tracers_ok(first, ntr):
            return EINVAL
        if wp is None:
            return EINVAL
        if eb is not None and eb != np.dtype(self.dtype).itemsize:
            return ESTATE
        if not self.uploaded:
            return ESTATE
        wp = np.asarray(wp)
        wp = wp.reshape(wp.shape + (1,)) if wp.ndim == 3 else wp
        blk = self.a["f"][sl0:sl0 + n, ..., first:first + ntr]
        new, psfc, pflux = sediment(blk, self.a["rho"][sl0:sl0 + n], self.a["adz"][sl0:sl0 + n], wp)
        self.a["f"][sl0:sl0 + n, ..., first:first + ntr] = new
        self._note()
        return psfc, pflux
