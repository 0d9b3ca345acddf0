"""The model of the eddy diffusion (include/mpdata_hip.h 3l) in plain numpy, the inputs its tests share, and the plan
model with the new call.

diffuse(f, rho, adz, tkh, cx, cz, sb, st): the arrays of ONE block in the reference layout -- f (n, nx+6, nzm[, T]), rho,
adz, cx, cz (n, nzm), tkh (n, nx+2, nzm), sb, st (n, nx) or None -- -> (f_new, zflux (n, nz[, T])).  Every numpy
operation below is one elementwise operation on arrays of f's dtype, hence one rounding per element, and the expressions
are parenthesised as the definition is; the sum of zflux is an explicit loop over i from +0.  Every f on the right is the
old one (f_new is a copy that only the last statement writes).  Only the interior columns 1 .. nx (array index 3 .. nx+2)
of f_new differ from f; columns 0 and nx+1 are read.
"""
import numpy as np

from oracle.plan_model import EINVAL, ESTATE, EUNSUPPORTED, PERIODIC, PlanModel
from util import bits


def diffuse(f, rho, adz, tkh, cx, cz, sb=None, st=None):
    f = np.asarray(f)
    dt = f.dtype
    one_tracer = f.ndim == 3
    F = f.reshape(f.shape + (1,)) if one_tracer else f
    n, nxp6, nzm, T = F.shape
    nx = nxp6 - 6
    for a, sh in ((rho, (n, nzm)), (adz, (n, nzm)), (cx, (n, nzm)), (cz, (n, nzm)), (tkh, (n, nx + 2, nzm))):
        assert np.asarray(a).dtype == dt and np.asarray(a).shape == sh, (np.asarray(a).dtype, np.asarray(a).shape, sh)
    for a in (sb, st):
        assert a is None or (np.asarray(a).dtype == dt and np.asarray(a).shape == (n, nx))
    tkh, cx, cz = np.asarray(tkh)[..., None], np.asarray(cx)[:, None, :, None], np.asarray(cz)[:, None, :, None]
    c = F[:, 2:nx + 4]                                      # columns 0 .. nx+1
    # Fx(i, k), i = 0 .. nx
    fx = -((cx * (tkh[:, :-1] + tkh[:, 1:])) * (c[:, 1:] - c[:, :-1]))
    # Fz(i, k'), i = 1 .. nx, interface k' = 0 .. nzm
    fz = np.zeros((n, nx, nzm + 1, T), dt)                  # +0.0: a NULL sb / st
    ci, ti = c[:, 1:-1], tkh[:, 1:-1]
    fz[:, :, 1:nzm] = -((cz[:, :, :-1] * (ti[:, :, :-1] + ti[:, :, 1:])) * (ci[:, :, 1:] - ci[:, :, :-1]))
    if sb is not None:
        fz[:, :, 0] = np.asarray(sb)[..., None]
    if st is not None:
        fz[:, :, nzm] = np.asarray(st)[..., None]
    ir = (dt.type(1) / (np.asarray(rho) * np.asarray(adz)))[:, None, :, None]
    out = np.array(F, order="F")
    out[:, 3:nx + 3] = ci - ((fx[:, 1:] - fx[:, :-1]) + (fz[:, :, 1:] - fz[:, :, :-1]) * ir)
    zflux = np.zeros((n, nzm + 1, T), dt)
    for i in range(nx):
        zflux = zflux + fz[:, i]
    for a in (fx, fz, ir, out, zflux):
        assert a.dtype == dt
    if one_tracer:
        out, zflux = out[..., 0], zflux[..., 0]
    return np.asfortranarray(out), np.asfortranarray(zflux)


# ---- inputs.  f: the raw signed fields of the oracle's generator (dist 3); halo columns come out of the same generator,
# so columns 0 and nx+1 differ from the interior.  tkh has a sharp k-gradient (a factor 16 between adjacent levels, odd
# against even, on top of noise), so a wrong k + 1 neighbour changes the result by far more than a rounding.  The
# coefficients are sized so that 2 cx max(tkh) 2 + 2 cz max(tkh) 2 ir <= 1 (the bound of the maximum principle):
# max(tkh) = 1, ir <= 1 / (0.5 * 0.5) = 4, cx <= 1 / 16, cz <= 1 / 64.
def make_coeffs(n, nx, nz, dtype, seed, fluxes=True):
    """{tkh, cx, cz, sb, st} of a block of n instances, Fortran order"""
    rng = np.random.default_rng([seed, n, nx, nz])
    nzm = nz - 1
    lev = np.where(np.arange(nzm) % 2 == 0, 1.0, 1.0 / 16.0)
    tkh = (rng.uniform(0.5, 1.0, (n, nx + 2, nzm)) * lev[None, None, :]).astype(dtype)
    cx = rng.uniform(1.0 / 32, 1.0 / 16, (n, nzm)).astype(dtype)
    cz = rng.uniform(1.0 / 128, 1.0 / 64, (n, nzm)).astype(dtype)
    out = dict(tkh=tkh, cx=cx, cz=cz, sb=None, st=None)
    if fluxes:
        out["sb"] = rng.uniform(-1.0 / 64, 1.0 / 64, (n, nx)).astype(dtype)
        out["st"] = rng.uniform(-1.0 / 64, 1.0 / 64, (n, nx)).astype(dtype)
    return {k: None if v is None else np.asfortranarray(v) for k, v in out.items()}


def make_plan_inputs(oracle, shape, T=1, dtype=np.float64, seed=100):
    """the seven arrays of a plan; rho and adz in [0.5, 1) so that ir <= 4"""
    kw = dict(dist=oracle.DIST_RAW_SIGNED, dtype=dtype)
    per = [oracle.make_inputs(*shape, seed=seed + t, **kw) for t in range(T)]
    inp = per[0]
    if T > 1:
        inp["f"] = np.asfortranarray(np.stack([p["f"] for p in per], axis=-1))
        inp["flux"] = np.asfortranarray(np.stack([p["flux"] for p in per], axis=-1))
    rng = np.random.default_rng([seed, 7])
    for k in ("rho", "adz"):
        inp[k] = np.asfortranarray(rng.uniform(0.5, 1.0, inp[k].shape).astype(dtype))
    return inp


class PlanModelDiffuse(PlanModel):
    """oracle.plan_model.PlanModel with section 3l.  The block rule: only instances [sl0, sl0 + n) and tracers [first,
    first + ntr) change.  The halo rule: a PERIODIC plan wraps the range's halos first (they are inputs) and the halos it
    then holds are those of the OLD field -- every read-back and run of the model wraps again, as the plan does after the
    call cleared its marks.  The phantom rule has no face here: the phantom of an odd fp32 plan is no instance, and it
    shows only through a later run of instance ncrms - 1, which the GPU tests compare.  `multi` / `windowed`: the kinds of
    handle the call refuses."""
    multi = False
    windowed = False

    def diffuse(self, tkh, cx, cz, sb=None, st=None, sl0=0, n=None, first=0, ntr=None, eb=None):
        ncrms, nx, nz, T = self.dims
        n = ncrms - sl0 if n is None else n
        ntr = T - first if ntr is None else ntr
        if n < 1 or sl0 < 0:
            return EINVAL
        if self.multi:
            return EUNSUPPORTED
        if sl0 + n > ncrms or not self._tracers_ok(first, ntr):
            return EINVAL
        if tkh is None or cx is None or cz is None:
            return EINVAL
        if self.windowed:
            return EUNSUPPORTED
        if eb is not None and eb != np.dtype(self.dtype).itemsize:
            return ESTATE
        if not self.uploaded:
            return ESTATE
        self._wrap(first, ntr)
        blk = self.a["f"][sl0:sl0 + n, ..., first:first + ntr]
        new, zflux = diffuse(blk, self.a["rho"][sl0:sl0 + n], self.a["adz"][sl0:sl0 + n], tkh, cx, cz, sb, st)
        self.a["f"][sl0:sl0 + n, ..., first:first + ntr] = new
        self._note()
        return zflux
