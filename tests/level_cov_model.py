"""The model of the per-level covariance of two tracers (include/mpdata_hip.h 3u) in plain numpy, the variants its tests
hold it against, the inputs the tests share, and the plan model with the new call.

level_cov(f, ta, tb, ma, mb, raw): the arrays of ONE block in the reference layout -- f (n, nx+6, nzm, T), ma, mb (n, nzm)
or None -- -> (cov, mean_a, mean_b), each (n, nzm) (raw: the means are None).  Every statement below is one elementwise
operation on arrays of f's dtype over (n, nzm), hence one rounding per element, in the definition's association; every sum
is an explicit loop over i = 1 .. nx from +0 (never np.sum, whose order is pairwise); the mean is ONE numpy division by nx in
f's dtype (numpy's division is the IEEE one).  Only the interior columns 1 .. nx (array index 3 .. nx+2) of tracers ta and
tb are read.  level_cov_loops is the same as scalar loops, statement by statement.

The variants (same signature, another arithmetic; none of them is the definition): reverse=True sums the columns from nx
down to 1 in every loop; recip=True forms the mean as s * (1 / nx) with the reciprocal rounded first; one_pass computes
sum(a b) - sum(a) sum(b) / nx.
"""
import numpy as np

from oracle.plan_model import EINVAL, ESTATE, EUNSUPPORTED, PlanModel

RAW = 1


def _cols(nx, reverse):
    return range(nx - 1, -1, -1) if reverse else range(nx)


def _mean(x, given, reverse=False, recip=False):
    """x (n, nx, nzm) -> the given profile, or s = +0; s = s + x_i; s / nx"""
    dt = x.dtype
    if given is not None:
        g = np.asarray(given)
        assert g.dtype == dt and g.shape == (x.shape[0], x.shape[2]), (g.dtype, g.shape)
        return np.array(g)
    nx = x.shape[1]
    s = np.zeros((x.shape[0], x.shape[2]), dt)              # +0
    for i in _cols(nx, reverse):
        s = s + x[:, i]
    if recip:
        return s * (dt.type(1) / dt.type(nx))
    return s / dt.type(nx)                                  # nx is exact in either precision; one rounded division


def level_cov(f, ta, tb, ma=None, mb=None, raw=False, reverse=False, recip=False):
    f = np.asarray(f)
    dt = f.dtype
    assert f.ndim == 4 and not (raw and (ma is not None or mb is not None))
    n, nxp6, nzm, T = f.shape
    nx = nxp6 - 6
    a = np.array(f[:, 3:nx + 3, :, ta])                     # columns 1 .. nx
    b = np.array(f[:, 3:nx + 3, :, tb])
    m_a = m_b = None
    if raw:
        da, db = a, b                                       # no subtraction at all
    else:
        m_a, m_b = _mean(a, ma, reverse, recip), _mean(b, mb, reverse, recip)
        da, db = a - m_a[:, None], b - m_b[:, None]
    c = np.zeros((n, nzm), dt)                              # +0
    for i in _cols(nx, reverse):
        p = da[:, i] * db[:, i]
        c = c + p
    for x in (da, db, c) + (() if raw else (m_a, m_b)):
        assert x.dtype == dt
    F = np.asfortranarray
    return F(c), None if raw else F(m_a), None if raw else F(m_b)


def level_cov_loops(f, ta, tb, ma=None, mb=None, raw=False):
    """the definition as scalar loops, one rounded operation per statement"""
    f = np.asarray(f)
    R = f.dtype.type
    n, nxp6, nzm, T = f.shape
    nx = nxp6 - 6
    cov, mean_a, mean_b = (np.zeros((n, nzm), f.dtype, order="F") for _ in range(3))
    for bi in range(n):
        for k in range(nzm):
            m = []
            for t, given in ((ta, ma), (tb, mb)):
                if raw:
                    m.append(None)
                elif given is not None:
                    m.append(given[bi, k])
                else:
                    s = R(0)
                    for i in range(3, nx + 3):
                        s = R(s + f[bi, i, k, t])
                    m.append(R(s / R(nx)))
            c = R(0)
            for i in range(3, nx + 3):
                a, b = f[bi, i, k, ta], f[bi, i, k, tb]
                da = a if raw else R(a - m[0])
                db = b if raw else R(b - m[1])
                p = R(da * db)
                c = R(c + p)
            cov[bi, k] = c
            if not raw:
                mean_a[bi, k], mean_b[bi, k] = m
    return cov, None if raw else mean_a, None if raw else mean_b


def one_pass(f, ta, tb):
    """sum(a b) - sum(a) sum(b) / nx, every statement rounded once: NOT the definition"""
    f = np.asarray(f)
    dt = f.dtype
    n, nxp6, nzm, T = f.shape
    nx = nxp6 - 6
    a, b = f[:, 3:nx + 3, :, ta], f[:, 3:nx + 3, :, tb]
    sab, sa, sb = (np.zeros((n, nzm), dt) for _ in range(3))
    for i in range(nx):
        sab = sab + a[:, i] * b[:, i]
        sa = sa + a[:, i]
        sb = sb + b[:, i]
    return np.asfortranarray(sab - sa * sb / dt.type(nx))


def long_two_pass(f, ta, tb, ma=None, mb=None, raw=False):
    """the two-pass evaluation in np.longdouble -> cov"""
    L = np.longdouble
    f = np.asarray(f)
    nx = f.shape[1] - 6
    a, b = f[:, 3:nx + 3, :, ta].astype(L), f[:, 3:nx + 3, :, tb].astype(L)
    if raw:
        da, db = a, b
    else:
        m_a = np.asarray(ma).astype(L) if ma is not None else sum(a[:, i] for i in range(nx)) / L(nx)
        m_b = np.asarray(mb).astype(L) if mb is not None else sum(b[:, i] for i in range(nx)) / L(nx)
        da, db = a - m_a[:, None], b - m_b[:, None]
    c = np.zeros(da[:, 0].shape, L)
    for i in range(nx):
        c = c + da[:, i] * db[:, i]
    return c


# ---- inputs.  f: the oracle's raw field moved by one half (subside_model.make_plan_inputs), so products and deviations
# take both signs.  Profiles ma, mb: uniform in [-0.25, 0.25), another value per instance and level.
def make_profile(n, nz, dtype=np.float64, seed=0, which=0):
    """(n, nzm), Fortran order"""
    rng = np.random.default_rng([seed, n, nz, 21 + which])
    return np.asfortranarray(rng.uniform(-0.25, 0.25, (n, nz - 1)).astype(dtype))


def make_plan_inputs(oracle, shape, T=3, dtype=np.float64, seed=100):
    import subside_model
    return subside_model.make_plan_inputs(oracle, shape, T, dtype, seed)


# the five ways the means of a central call come about, and RAW: name -> (ma given, mb given, raw)
MEANS = {"raw": (False, False, True), "central": (False, False, False), "ma": (True, False, False), "mb": (False, True, False),
         "both": (True, True, False)}


def call_args(n, nz, dtype, seed, how):
    """(ma, mb, raw) of a call of kind `how` (a key of MEANS) on n instances"""
    ga, gb, raw = MEANS[how]
    return (make_profile(n, nz, dtype, seed, 0) if ga else None, make_profile(n, nz, dtype, seed, 1) if gb else None, raw)


def share_differs(x, y):
    """the share of the elements of x and y that differ in bits"""
    from util import bits
    return float(np.mean(bits(x) != bits(y)))


class PlanModelLevelCov(PlanModel):
    """oracle.plan_model.PlanModel with section 3u.  The call reads the interior columns of tracers ta and tb of instances
    [sl0, sl0 + n) and changes NOTHING of the model: no array, no flag, no bookkeeping.  The error order: the block (n,
    sl0), the handle, the range, the pair, the mode bits, RAW with a profile or a mean output, the NULL cov, the precision
    of a host form, the state.  Halo columns are not read, so the boundary mode has no face here; the model holds the tall
    column, which is what the owners of a windowed plan hold."""
    multi = False

    def level_cov(self, ta, tb, ma=None, mb=None, mode=0, sl0=0, n=None, eb=None, cov=True, mean_a=False, mean_b=False):
        """cov, mean_a, mean_b: whether the call passes the output -> (cov, mean_a or None, mean_b or None), or the code"""
        ncrms, nx, nz, T = self.dims
        n = ncrms - sl0 if n is None else n
        if n < 1 or sl0 < 0:
            return EINVAL
        if self.multi:
            return EUNSUPPORTED
        if sl0 + n > ncrms:
            return EINVAL
        if not (0 <= ta < T and 0 <= tb < T):
            return EINVAL
        if mode & ~RAW:
            return EINVAL
        if mode & RAW and (ma is not None or mb is not None or mean_a or mean_b):
            return EINVAL
        if not cov:
            return EINVAL
        if eb is not None and eb != np.dtype(self.dtype).itemsize:
            return ESTATE
        if not self.uploaded:
            return ESTATE
        c, m_a, m_b = level_cov(self.a["f"][sl0:sl0 + n], ta, tb, ma, mb, bool(mode & RAW))
        return c, m_a if mean_a else None, m_b if mean_b else None
