"""The model of the implicit vertical diffusion with a per-cell diffusivity (include/mpdata_hip.h 3s) in plain numpy, the
inputs its tests share, and the plan model with the new call.

vdiffuse(f, rho, adz, tkh, cz, sb, st): the arrays of ONE block in the reference layout -- f (n, nx+6, nzm[, T]), rho, adz,
cz (n, nzm), tkh (n, nx+2, nzm), sb, st (n, nx) or None -- -> f_new.  Vectorised over (instance, column[, tracer]),
sequential in k; every statement below is one elementwise operation on arrays of f's dtype, hence one rounding per
element, in the definition's order and association.  Every f on the right is the old one.  Only the interior columns
1 .. nx (array index 3 .. nx+2) of f_new differ from f; halo columns of f, columns 0 and nx+1 of tkh and cz[:, nzm-1] are
not read.  coefficients(...) returns the a, c, di of the section, for the tests that hand them to vsolve_model.
"""
import numpy as np

from oracle.plan_model import EINVAL, ESTATE, EUNSUPPORTED, PlanModel


def coefficients(rho, adz, tkh, cz):
    """-> (ir (n, nzm), a, c, di (n, nx, nzm)) of the interior columns"""
    rho, adz, tkh, cz = (np.asarray(x) for x in (rho, adz, tkh, cz))
    dt = rho.dtype
    n, nzm = rho.shape
    nx = tkh.shape[1] - 2
    one = dt.type(1)
    prod = rho * adz
    ir = one / prod
    ti = tkh[:, 1:nx + 1]                                   # columns 1 .. nx
    e = np.zeros((n, nx, nzm + 1), dt)                      # e[..., k] = e(i,k), k = 0 .. nzm; e(i,0) = e(i,nzm) = +0
    for k in range(1, nzm):
        s = ti[:, :, k - 1] + ti[:, :, k]
        e[:, :, k] = cz[:, None, k - 1] * s
        assert s.dtype == dt
    a = e[:, :, :-1] * ir[:, None, :]
    c = e[:, :, 1:] * ir[:, None, :]
    t = one + a
    di = t + c
    for x in (prod, ir, e, a, c, t, di):
        assert x.dtype == dt
    return ir, a, c, di


def vdiffuse(f, rho, adz, tkh, cz, sb=None, st=None):
    f = np.asarray(f)
    dt = f.dtype
    one_tracer = f.ndim == 3
    F = f.reshape(f.shape + (1,)) if one_tracer else f
    n, nxp6, nzm, T = F.shape
    nx = nxp6 - 6
    for x, sh in ((rho, (n, nzm)), (adz, (n, nzm)), (cz, (n, nzm)), (tkh, (n, nx + 2, nzm))):
        assert np.asarray(x).dtype == dt and np.asarray(x).shape == sh, (np.asarray(x).dtype, np.asarray(x).shape, sh)
    for x in (sb, st):
        assert x is None or (np.asarray(x).dtype == dt and np.asarray(x).shape == (n, nx))
    one = dt.type(1)
    ir, a, c, di = coefficients(rho, adz, tkh, cz)
    a, c, di = a[..., None], c[..., None], di[..., None]    # (n, nx, nzm, 1): shared by the tracers
    r = np.array(F[:, 3:nx + 3])                            # columns 1 .. nx
    if sb is not None:
        pr = np.asarray(sb) * ir[:, None, 0]
        r[:, :, 0] = r[:, :, 0] + pr[..., None]
        assert pr.dtype == dt
    if st is not None:
        pr = np.asarray(st) * ir[:, None, nzm - 1]
        r[:, :, nzm - 1] = r[:, :, nzm - 1] - pr[..., None]
        assert pr.dtype == dt
    g = np.zeros((n, nx, nzm, 1), dt)
    y = np.empty_like(r)
    p = one / di[:, :, 0]
    g[:, :, 0] = c[:, :, 0] * p
    y[:, :, 0] = r[:, :, 0] * p
    for k in range(1, nzm):
        m = a[:, :, k] * g[:, :, k - 1]
        d = di[:, :, k] - m
        p = one / d
        g[:, :, k] = c[:, :, k] * p
        q = a[:, :, k] * y[:, :, k - 1]
        v = r[:, :, k] + q
        y[:, :, k] = v * p
        for x in (m, d, p, q, v):
            assert x.dtype == dt
    x = np.empty_like(y)
    x[:, :, nzm - 1] = y[:, :, nzm - 1]
    for k in range(nzm - 2, -1, -1):
        m = g[:, :, k] * x[:, :, k + 1]
        x[:, :, k] = y[:, :, k] + m
        assert m.dtype == dt
    out = np.array(F, order="F")
    out[:, 3:nx + 3] = x
    assert out.dtype == dt and g.dtype == dt and y.dtype == dt
    return np.asfortranarray(out[..., 0] if one_tracer else out)


# ---- inputs.  tkh: uniform in [0, 1) in "cloudy" cells, exactly zero beside them (about a third of the cells, and a whole
# column now and then), every column and instance its own; cz uniform in [0, 2); with rho, adz in [0.5, 1) the off-diagonals
# cz (tkh + tkh) ir reach 16.  sb, st uniform in [-1/64, 1/64).  The matrix has row sums 1 and non-positive off-diagonals:
# max|x| <= max|r|, so chains of calls and runs stay finite.
def make_coeffs(n, nx, nz, dtype=np.float64, seed=0, fluxes=True, x_uniform=False):
    """{tkh, cz, sb, st} of a block of n instances, Fortran order"""
    rng = np.random.default_rng([seed, n, nx, nz, 11])
    nzm = nz - 1
    tkh = rng.uniform(0.0, 1.0, (n, nx + 2, nzm))
    tkh[rng.uniform(0.0, 1.0, tkh.shape) < 1.0 / 3] = 0.0
    tkh[rng.uniform(0.0, 1.0, (n, nx + 2)) < 1.0 / 8] = 0.0
    if x_uniform:
        tkh[:] = tkh[:, 1:2]
    out = dict(tkh=tkh.astype(dtype), cz=rng.uniform(0.0, 2.0, (n, nzm)).astype(dtype), sb=None, st=None)
    if fluxes:
        out["sb"] = rng.uniform(-1.0 / 64, 1.0 / 64, (n, nx)).astype(dtype)
        out["st"] = rng.uniform(-1.0 / 64, 1.0 / 64, (n, nx)).astype(dtype)
    return {k: None if v is None else np.asfortranarray(v) for k, v in out.items()}


def make_plan_inputs(oracle, shape, T=1, dtype=np.float64, seed=100):
    """the seven arrays of a plan, as subside_model.make_plan_inputs makes them: f signed, in [-0.5, 0.5); rho and adz
    in [0.5, 1); f and flux carry a tracer axis only for T > 1"""
    import subside_model
    return subside_model.make_plan_inputs(oracle, shape, T, dtype, seed)


class PlanModelVdiffuse(PlanModel):
    """oracle.plan_model.PlanModel with section 3s.  The block rule: only instances [sl0, sl0 + n) and tracers [first,
    first + ntr) change.  The error order: the block, the handle, the range, the tracers, the NULL tkh or cz, a windowed
    plan, the precision of a host form, the state.  The interior-only rule: halo columns are neither read nor written.
    The periodic rule: no wrap is part of the call; the halos a PERIODIC model then holds are those of the OLD field, and
    every read-back and run of the model wraps again, as the plan does after the call cleared its marks.  `multi` /
    `windowed`: the kinds of handle the call refuses."""
    multi = False
    windowed = False

    def vdiffuse(self, tkh, cz, sb=None, st=None, sl0=0, n=None, first=0, ntr=None, eb=None):
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
        if tkh is None or cz is None:
            return EINVAL
        if self.windowed:
            return EUNSUPPORTED
        if eb is not None and eb != np.dtype(self.dtype).itemsize:
            return ESTATE
        if not self.uploaded:
            return ESTATE
        blk = self.a["f"][sl0:sl0 + n, ..., first:first + ntr]
        self.a["f"][sl0:sl0 + n, ..., first:first + ntr] = vdiffuse(blk, self.a["rho"][sl0:sl0 + n], self.a["adz"][sl0:sl0 + n],
                                                                    tkh, cz, sb, st)
        self._note()
        return None
