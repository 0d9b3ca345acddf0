"""The model of the large-scale vertical advection (include/mpdata_hip.h 3m) in plain numpy, the inputs its tests share,
and the plan model with the new call.

subside(f, cb, cc): the arrays of ONE block in the reference layout -- f (n, nx+6, nzm[, T]), cb, cc (n, nzm) -- ->
(f_new, dsum (n, nzm[, T])).  Every statement below is one elementwise operation on arrays of f's dtype, hence one
rounding per element, in the definition's association: two subtractions, two products, their sum, the final subtraction;
the sum of dsum is an explicit loop over i = 1 .. nx from +0.  Every f on the right is the old one.  EVERY column slot is
updated, the halo columns included.
"""
import numpy as np

from oracle.plan_model import EINVAL, ESTATE, EUNSUPPORTED, PlanModel
from util import bits


def subside(f, cb, cc):
    f = np.asarray(f)
    dt = f.dtype
    one_tracer = f.ndim == 3
    F = f.reshape(f.shape + (1,)) if one_tracer else f
    n, nxp6, nzm, T = F.shape
    nx = nxp6 - 6
    for a in (cb, cc):
        assert np.asarray(a).dtype == dt and np.asarray(a).shape == (n, nzm), (np.asarray(a).dtype, np.asarray(a).shape)
    cb, cc = np.asarray(cb)[:, None, :, None], np.asarray(cc)[:, None, :, None]
    k = np.arange(nzm)
    fd = F[:, :, np.maximum(k - 1, 0)]           # f(i, kb)
    fu = F[:, :, np.minimum(k + 1, nzm - 1)]     # f(i, kc)
    a = F - fd
    c = fu - F
    pa = cb * a
    pc = cc * c
    dec = pa + pc
    out = F - dec
    dsum = np.zeros((n, nzm, T), dt)             # +0
    for i in range(nx):
        dsum = dsum + dec[:, 3 + i]
    for x in (a, c, pa, pc, dec, out, dsum):
        assert x.dtype == dt
    if one_tracer:
        out, dsum = out[..., 0], dsum[..., 0]
    return np.asfortranarray(out), np.asfortranarray(dsum)


# ---- inputs.  cb, cc: random, of both signs, another value per instance and level, |.| < 0.3 so that a chain of calls
# and runs stays bounded (|f_new| <= 2.2 max|f|).
def make_coeffs(n, nz, dtype, seed):
    """(cb, cc) of a block of n instances, Fortran order"""
    rng = np.random.default_rng([seed, n, nz])
    return tuple(np.asfortranarray(rng.uniform(-0.3, 0.3, (n, nz - 1)).astype(dtype)) for _ in range(2))


def make_plan_inputs(oracle, shape, T=1, dtype=np.float64, seed=100):
    """the seven arrays of a plan; f: the oracle's raw field moved by one half, so signed, in [-0.5, 0.5); rho and adz in
    [0.5, 1); f and flux carry a tracer axis only for T > 1"""
    kw = dict(dist=oracle.DIST_RAW_SIGNED, dtype=dtype)
    per = [oracle.make_inputs(*shape, seed=seed + t, **kw) for t in range(T)]
    inp = per[0]
    if T > 1:
        inp["f"] = np.asfortranarray(np.stack([p["f"] for p in per], axis=-1))
        inp["flux"] = np.asfortranarray(np.stack([p["flux"] for p in per], axis=-1))
    inp["f"] = np.asfortranarray(inp["f"] - np.dtype(dtype).type(0.5))
    assert inp["f"].dtype == np.dtype(dtype)
    rng = np.random.default_rng([seed, 7])
    for k in ("rho", "adz"):
        inp[k] = np.asfortranarray(rng.uniform(0.5, 1.0, inp[k].shape).astype(dtype))
    return inp


class PlanModelSubside(PlanModel):
    """oracle.plan_model.PlanModel with section 3m.  The block rule: only instances [sl0, sl0 + n) and tracers [first,
    first + ntr) change.  The error order: the block, the handle, the range, the tracers, the NULLs, the precision of a
    host form, the state.  The wrap rule: the call acts on every column alike and launches no wrap -- the model applies
    the operator to the halo columns it holds; a PERIODIC model wraps on every read-back and run as before, and wrapping
    commutes with an operator that is the same in every column.  Windows, seams and the phantom have no face here: a
    windowed plan must hold what the tall model holds."""
    multi = False

    def subside(self, cb, cc, sl0=0, n=None, first=0, ntr=None, eb=None):
        ncrms, nx, nz, T = self.dims
        n = ncrms - sl0 if n is None else n
        ntr = T - first if ntr is None else ntr
        if n < 1 or sl0 < 0:
            return EINVAL
        if self.multi:
            return EUNSUPPORTED
        if sl0 + n > ncrms or not self._tracers_ok(first, ntr):
            return EINVAL
        if cb is None or cc is None:
            return EINVAL
        if eb is not None and eb != np.dtype(self.dtype).itemsize:
            return ESTATE
        if not self.uploaded:
            return ESTATE
        new, dsum = subside(self.a["f"][sl0:sl0 + n, ..., first:first + ntr], cb, cc)
        self.a["f"][sl0:sl0 + n, ..., first:first + ntr] = new
        self._note()
        return dsum
