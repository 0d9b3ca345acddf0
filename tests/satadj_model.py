"""The model of the saturation adjustment (include/mpdata_hip.h 3y) in plain numpy, the test curve, the inputs its tests
share, and the plan model with the new call.

satadj(f, th, tq, tn, tt, pres, gz, par, ice): the arrays of ONE block in the reference layout -- f (n, nx+6, nzm, T), pres
(n, nzm), gz (n, nzm) or None, par a dict of Python numbers (PAR) -- -> (f_new, ncld (n, nzm), iters (n, nzm)).  Every
statement is one elementwise operation on arrays of f's dtype, hence one rounding per element, in the definition's
association; the comparisons are np.where on a plain `>` / `>=` / `<=`, so NaN and -0 take the "else" value; the Newton
loop is masked: every cell is evaluated while any cell is active, and a cell that has stopped keeps its T, qs, dq and d.
Rows with pres == 0 are copied, not computed.  Only the interior columns 1 .. nx (array index 3 .. nx+2) of tracers tn and
tt of f_new differ from f; halo columns and other tracers are not read.  satadj_loops is the same as a scalar triple loop,
statement by statement.
"""
import numpy as np

from oracle.plan_model import EINVAL, ESTATE, EUNSUPPORTED, PlanModel

ICE = 1

# ---- the test curve: data of this module, the test's curve and nothing more (no physical accuracy is under test)
PAR = dict(
    esw=[6.11239921, 0.443987641, 0.142986287e-1, 0.264847430e-3, 0.302950461e-5, 0.206739458e-7, 0.640689451e-10,
         -0.952447341e-13, -0.976195544e-15],
    desw=[0.443956472, 0.285976452e-1, 0.794747212e-3, 0.121167162e-4, 0.103167413e-6, 0.385208005e-9, -0.604119582e-12,
          -0.792933209e-14, -0.599634321e-17],
    esi=[6.11147274, 0.503160820, 0.188439774e-1, 0.420895665e-3, 0.615021634e-5, 0.602588177e-7, 0.385852041e-9,
         0.146898966e-11, 0.252751365e-14],
    desi=[0.503223089, 0.377174432e-1, 0.126710138e-2, 0.249065913e-4, 0.312668753e-6, 0.255653718e-8, 0.132073448e-10,
          0.390204672e-13, 0.497275778e-16],
    t0=273.16, xmin=-80.0, eps=0.622, lv=2.5104e6 / 1004, ls=2.8440e6 / 1004, tmin=253.16, tmax=273.16, tol=0.01, maxit=10)


def par_with(**kw):
    """PAR with some entries replaced"""
    p = dict(PAR)
    p.update(kw)
    return p


class _P:
    """the numbers of par in the dtype: each rounded once; an, bn, lf formed in the dtype, each operation rounded once"""

    def __init__(self, par, dt):
        R = np.dtype(dt).type
        with np.errstate(all="ignore"):
            for k in ("esw", "desw", "esi", "desi"):
                setattr(self, k, [R(v) for v in par[k]])
            for k in ("t0", "xmin", "eps", "lv", "ls", "tmin", "tmax", "tol"):
                setattr(self, k, R(par[k]))
            self.maxit = int(par["maxit"])
            self.an = R(R(1) / R(self.tmax - self.tmin))
            self.bn = R(self.tmin * self.an)
            self.lf = R(self.ls - self.lv)


class Watch:
    """what the tests assert of the intermediates: the values a cell USES are finite and not subnormal"""

    def __init__(self, dt):
        self.tiny = np.finfo(dt).tiny
        self.nonfinite = 0
        self.subnormal = 0

    def see(self, mask, *arrs):
        for a in arrs:
            v = np.broadcast_to(a, mask.shape)[mask]
            self.nonfinite += int(np.count_nonzero(~np.isfinite(v)))
            self.subnormal += int(np.count_nonzero((v != 0) & (np.abs(v) < self.tiny)))


def _curve(c, dc, T, p, rp, P, need, watch):
    x = T - P.t0
    x = np.where(x > P.xmin, x, P.xmin)
    es = np.full(T.shape, c[8], T.dtype)
    de = np.full(T.shape, dc[8], T.dtype)
    for j in range(7, -1, -1):
        xe, xd = x * es, x * de
        es, de = c[j] + xe, dc[j] + xd
        if watch is not None:
            watch.see(need, xe, xd, es, de)
    pm = p - es
    den = np.where(pm > es, pm, es)
    num = P.eps * es
    qs = num / den
    nd = P.eps * de
    dq = nd * rp
    if watch is not None:
        watch.see(need, x, pm, num, qs, nd, dq)
    return qs, dq


def _sat(T, p, rp, P, ice, need, watch=None):
    """-> (qs, dq, L, dL, regime) with regime 0 liquid, 1 ice, 2 mixed; need: the cells whose result is used"""
    dt = T.dtype
    zero = dt.type(0)
    if not ice:
        qs, dq = _curve(P.esw, P.desw, T, p, rp, P, need, watch)
        return qs, dq, np.full(T.shape, P.lv, dt), np.full(T.shape, zero, dt), np.zeros(T.shape, np.int8)
    isw = T >= P.tmax
    isi = ~isw & (T <= P.tmin)
    qw, dw = _curve(P.esw, P.desw, T, p, rp, P, need & ~isi, watch)
    qi, di = _curve(P.esi, P.desi, T, p, rp, P, need & ~isw, watch)
    om = P.an * T
    om = om - P.bn
    u = dt.type(1) - om
    a1, a2 = om * qw, u * qi
    qm = a1 + a2
    b1, b2 = om * dw, u * di
    dm = b1 + b2
    ul = u * P.lf
    lm = P.lv + ul
    dlm = dt.type(P.an * P.lf)
    if watch is not None:
        watch.see(need & ~isw & ~isi, om, u, a1, a2, qm, b1, b2, dm, ul, lm)
    qs = np.where(isw, qw, np.where(isi, qi, qm))
    dq = np.where(isw, dw, np.where(isi, di, dm))
    L = np.where(isw, P.lv, np.where(isi, P.ls, lm)).astype(dt)
    dL = np.where(isw | isi, zero, dlm).astype(dt)
    return qs, dq, L, dL, np.where(isw, 0, np.where(isi, 1, 2)).astype(np.int8)


def qsat(T, p, par=PAR, ice=False):
    """qs(T) of the definition at pressure p, elementwise in T's dtype (what the field makers and the planted cells use)"""
    T = np.asarray(T)
    P = _P(par, T.dtype)
    p = np.asarray(p, T.dtype)
    with np.errstate(all="ignore"):
        return _sat(T, p, T.dtype.type(1) / p, P, ice, np.ones(T.shape, bool))[0]


def satadj(f, th, tq, tn, tt, pres, gz=None, par=PAR, ice=False, parts=False):
    """-> (f_new, ncld, iters); parts: -> (f_new, ncld, iters, info) with info a dict of (n, nx, nzm) arrays -- on (the row
    is computed), wet (the cell iterates), it, regime (of the last sat), T1, qs1 = qs(T1) -- and watch, a Watch"""
    f = np.asarray(f)
    dt = f.dtype
    assert f.ndim == 4 and len({th, tq, tn} | ({tt} if tt >= 0 else set())) == (4 if tt >= 0 else 3)
    n, nxp6, nzm, T_ = f.shape
    nx = nxp6 - 6
    zero = dt.type(0)
    P = _P(par, dt)
    for x in (pres, gz):
        assert x is None or (np.asarray(x).dtype == dt and np.asarray(x).shape == (n, nzm)), (x.dtype, x.shape, (n, nzm))
    watch = Watch(dt)
    with np.errstate(all="ignore"):
        h = np.array(f[:, 3:nx + 3, :, th])                    # columns 1 .. nx
        q = np.array(f[:, 3:nx + 3, :, tq])
        p = np.broadcast_to(np.asarray(pres)[:, None, :], h.shape)
        on = p != 0
        rp = dt.type(1) / p
        qq = np.where(q > 0, q, zero)
        T1 = h - np.asarray(gz)[:, None, :] if gz is not None else h
        qs, dq, L, dL, reg = _sat(T1, p, rp, P, ice, on, watch)
        qs1 = qs
        T = np.array(T1)
        wet = on & (qq > qs)
        act = np.array(wet)
        it = np.zeros(h.shape, np.int32)
        d = np.zeros(h.shape, dt)
        while act.any():
            nqs, ndq, L, dL, nreg = _sat(T, p, rp, P, ice, act, watch)
            e = qq - nqs
            le = L * e
            fff = (T1 - T) + le
            de_, ldq = dL * e, L * ndq
            dfff = (de_ - ldq) - dt.type(1)
            nd = (-fff) / dfff
            nT = T + nd
            watch.see(act, e, le, fff, ldq, dfff, nd, nT)
            watch.see(act & (dL != 0), de_)
            qs = np.where(act, nqs, qs)
            dq = np.where(act, ndq, dq)
            d = np.where(act, nd, d)
            T = np.where(act, nT, T)
            reg = np.where(act, nreg, reg)
            it = np.where(act, it + 1, it)
            act = act & (np.abs(nd) > P.tol) & (it < P.maxit)
        dd = dq * d
        qe = qs + dd
        v = qq - qe
        watch.see(wet, dd, qe, v)
        v = np.where(v > 0, v, zero)
        qn = np.where(wet, v, zero)
    for x in (qn, T, qs, dq, d):
        assert x.dtype == dt
    out = np.array(f, order="F")
    out[:, 3:nx + 3, :, tn] = np.where(on, qn, f[:, 3:nx + 3, :, tn])
    if tt >= 0:
        out[:, 3:nx + 3, :, tt] = np.where(on, T, f[:, 3:nx + 3, :, tt])
    ncld = np.asfortranarray(np.sum(on & (qn > 0), axis=1).astype(dt))
    iters = np.asfortranarray(np.max(np.where(on, it, 0), axis=1).astype(dt))
    if parts:
        return np.asfortranarray(out), ncld, iters, dict(on=on, wet=wet, it=it, regime=reg, T1=T1, qs1=qs1, watch=watch)
    return np.asfortranarray(out), ncld, iters


def satadj_loops(f, th, tq, tn, tt, pres, gz=None, par=PAR, ice=False):
    """the definition as scalar loops, one rounded operation per statement -> (f_new, ncld, iters, it (n, nx, nzm))"""
    f = np.asarray(f)
    R = f.dtype.type
    n, nxp6, nzm, T_ = f.shape
    nx = nxp6 - 6
    P = _P(par, f.dtype)
    out = np.array(f, order="F")
    ncld, iters = np.zeros((n, nzm), f.dtype, order="F"), np.zeros((n, nzm), f.dtype, order="F")
    its = np.zeros((n, nx, nzm), np.int32)

    def curve(c, dc, T, p, rp):
        x = R(T - P.t0)
        x = x if x > P.xmin else P.xmin
        es, de = c[8], dc[8]
        for j in range(7, -1, -1):
            es = R(c[j] + R(x * es))
            de = R(dc[j] + R(x * de))
        pm = R(p - es)
        den = pm if pm > es else es
        return R(R(P.eps * es) / den), R(R(P.eps * de) * rp)

    def sat(T, p, rp):
        if not ice or T >= P.tmax:
            return curve(P.esw, P.desw, T, p, rp) + (P.lv, R(0))
        if T <= P.tmin:
            return curve(P.esi, P.desi, T, p, rp) + (P.ls, R(0))
        om = R(R(P.an * T) - P.bn)
        u = R(R(1) - om)
        qw, dw = curve(P.esw, P.desw, T, p, rp)
        qi, di = curve(P.esi, P.desi, T, p, rp)
        return (R(R(om * qw) + R(u * qi)), R(R(om * dw) + R(u * di)), R(P.lv + R(u * P.lf)), R(P.an * P.lf))

    with np.errstate(all="ignore"):
        for b in range(n):
            for k in range(nzm):
                p = pres[b, k]
                if p == 0:
                    continue
                rp = R(R(1) / p)
                cnt, itmax = 0, 0
                for i in range(3, nx + 3):
                    h, q = f[b, i, k, th], f[b, i, k, tq]
                    qq = q if q > 0 else R(0)
                    T1 = R(h - gz[b, k]) if gz is not None else h
                    qs = sat(T1, p, rp)[0]
                    T = T1
                    it = 0
                    if qq > qs:
                        while True:
                            qs, dq, L, dL = sat(T, p, rp)
                            e = R(qq - qs)
                            fff = R(R(T1 - T) + R(L * e))
                            dfff = R(R(R(dL * e) - R(L * dq)) - R(1))
                            d = R(R(-fff) / dfff)
                            T = R(T + d)
                            it += 1
                            if not (abs(d) > P.tol and it < P.maxit):
                                break
                        qs = R(qs + R(dq * d))
                        qn = R(qq - qs)
                        qn = qn if qn > 0 else R(0)
                    else:
                        qn = R(0)
                    out[b, i, k, tn] = qn
                    if tt >= 0:
                        out[b, i, k, tt] = T
                    cnt += bool(qn > 0)
                    itmax = max(itmax, it)
                    its[b, i - 3, k] = it
                ncld[b, k], iters[b, k] = cnt, itmax
    return out, ncld, iters, its


# ---- the conditions every test asserts on the model for the rows it touches (conditions, not measurements)
def check_conditions(info, ice, maxit, planted=None, rows_differ=True):
    """info: the parts of a satadj call of the model.  The saturated share is in [0.15, 0.6]; with ICE each regime holds at
    least 10 % of the saturated cells; the most steps are <= 7 where maxit is 10; somewhere two cells of one row differ in
    it (wherever maxit >= 2: the barely saturated cells of fill_fields take one step); with maxit == 2 at least 30 % of the saturated cells end at the cap; no intermediate a cell uses is non-finite or
    subnormal; the planted cells (q == qs(T1) exactly) are dry; at least one row has pres == 0.
    rows_differ False: a row has one cell (nx == 1) and cannot hold two values of it."""
    on, wet, it, reg = info["on"], info["wet"], info["it"], info["regime"]
    assert on.any() and not on.all(), "no row with pres == 0, or no other"
    share = wet[on].mean()
    assert 0.15 <= share <= 0.6, share
    if ice:
        for r in range(3):
            assert (reg[wet] == r).mean() >= 0.10, (r, (reg[wet] == r).mean())
    if maxit == 10:
        assert it.max() <= 7, it.max()
    if maxit >= 2 and rows_differ:
        lo = np.where(wet, it, 99).min(axis=1)
        hi = np.where(wet, it, 0).max(axis=1)
        assert ((wet.sum(axis=1) >= 2) & (hi > lo)).any(), "no row whose cells differ in it"
    if maxit == 2:
        assert (it[wet] == 2).mean() >= 0.30, (it[wet] == 2).mean()
    w = info["watch"]
    assert w.nonfinite == 0 and w.subnormal == 0, (w.nonfinite, w.subnormal)
    if planted is not None:
        assert planted.any() and not wet[planted].any()


# ---- inputs.  The recipe: p uniform in [150, 1010] per row; T1 = 225 + 80 (p - 150) / 860 + U(-6, 6) per cell (a T1 tied to
# p: one that is not makes some cells fail to converge); q = U(0, 1.6) * qs(T1), every seventh cell negated; h = T1 + gz.
def make_rows(n, nz, dtype=np.float64, seed=0, zero_rows=True):
    """pres, gz (n, nzm), Fortran order; zero_rows: pres == 0 on every fifth row, counted along the array, from the second"""
    rng = np.random.default_rng([seed, n, nz, 31])
    nzm = nz - 1
    pres = rng.uniform(150.0, 1010.0, (n, nzm)).astype(dtype)
    gz = rng.uniform(0.0, 120.0, (n, nzm)).astype(dtype)
    if zero_rows:
        pres.reshape(-1)[1::5] = 0
    return np.asfortranarray(pres), np.asfortranarray(gz)


def fill_fields(f, th, tq, pres, gz=None, par=PAR, ice=False, seed=0, plant=True, after=None):
    """f (n, nx+6, nzm, T) with the interior columns of tracers th and tq set by the recipe for the rows pres, gz (the
    block's; gz None: h = T1) -> (f_new, planted (n, nx, nzm)): on the planted cells (column 2 of every third level, or column 1 of every ninth where nx == 1, where
    pres != 0) q is qs(T1) exactly, with T1 as the call forms it.  Rows with pres == 0 are filled as if p were 500.  Some cells sit on the edges
    of the mixed-phase ramp exactly (below).  after: a function of the interior h (n, nx, nzm) -> the h the call will meet, where
    another call changes th between the import of f and the adjustment: q, the planted and the barely saturated cells are then
    made for that h (no cell is put on the edges of the ramp), and f still holds the h of before."""
    f = np.array(f, order="F")
    dt = f.dtype
    n, nxp6, nzm, T_ = f.shape
    nx = nxp6 - 6
    rng = np.random.default_rng([seed, n, nx, nzm, 32])
    p = np.where(np.asarray(pres) != 0, pres, dt.type(500)).astype(np.float64)[:, None, :]
    T1 = 225.0 + 80.0 * (p - 150.0) / 860.0 + rng.uniform(-6.0, 6.0, (n, nx, nzm))
    g = np.asarray(gz, np.float64)[:, None, :] if gz is not None else 0.0
    h = (T1 + g).astype(dt)
    hc = h if after is None else after(h)
    assert hc.dtype == dt and hc.shape == h.shape
    T1r = hc - np.asarray(gz)[:, None, :] if gz is not None else hc         # as the call forms it
    qs = qsat(T1r, p.astype(dt), par, ice)
    q = (rng.uniform(0.0, 1.6, (n, nx, nzm)) * qs.astype(np.float64)).astype(dt)
    neg = np.zeros(q.size, bool)
    neg[6::7] = True
    q = np.where(neg.reshape(q.shape), -q, q)
    planted = np.zeros(q.shape, bool)
    if plant:
        planted[:, min(1, nx - 1), ::3 if nx > 1 else 9] = True
        planted &= np.broadcast_to((np.asarray(pres) != 0)[:, None, :], q.shape)
        q = np.where(planted, qs, q)
    # cells on the edges of the ramp: T1 == tmax exactly (T1 == tmin on every second such row) with q = 1.3 qs(T1), in the
    # last column of the rows whose recipe holds that temperature (the centre within 6 of it), where h - gz gives it exactly
    P = _P(par, dt)
    centre = 225.0 + 80.0 * (p[:, 0, :] - 150.0) / 860.0
    for b, k in zip(*np.nonzero(np.asarray(pres) != 0)):
        edge = P.tmin if (b + k) % 2 else P.tmax
        if not plant or after is not None or planted[b, nx - 1, k] or abs(centre[b, k] - float(edge)) > 6.0:
            continue
        hh = edge if gz is None else dt.type(edge + gz[b, k])
        for _ in range(4):
            back = hh if gz is None else dt.type(hh - gz[b, k])
            if back == edge:
                break
            hh = np.nextafter(hh, dt.type(np.inf) if back < edge else dt.type(-np.inf))
        else:
            continue
        h[b, nx - 1, k] = hh
        q[b, nx - 1, k] = dt.type(1.3) * qsat(np.array([edge], dt), np.array([pres[b, k]], dt), par, ice)[0]
    # barely saturated cells: q = qs(T1) (1 + 1e-4) in column 1 of every third level from the second (nx >= 2), so that d of
    # the first step is below tol and the cell takes ONE step: under maxit = 2 nearly every other saturated cell takes two,
    # and a row must hold two values of it
    if plant and nx >= 2:
        barely = np.zeros(q.shape, bool)
        barely[:, 0, 1::3] = True
        barely &= np.broadcast_to((np.asarray(pres) != 0)[:, None, :], q.shape) & ~planted
        q = np.where(barely, (qs.astype(np.float64) * (1.0 + 1e-4)).astype(dt), q)
    f[:, 3:nx + 3, :, th] = h
    f[:, 3:nx + 3, :, tq] = q
    return np.asfortranarray(f), planted


def edge_cells(f, th, pres, gz=None, par=PAR):
    """the interior cells of a block with T1 == tmax or T1 == tmin exactly, on rows with pres != 0 -> a count"""
    nx = f.shape[1] - 6
    P = _P(par, f.dtype)
    h = f[:, 3:nx + 3, :, th]
    T1 = h - np.asarray(gz)[:, None, :] if gz is not None else h
    on = np.broadcast_to((np.asarray(pres) != 0)[:, None, :], T1.shape)
    return int(np.count_nonzero(on & ((T1 == P.tmax) | (T1 == P.tmin))))


class PlanModelSatadj(PlanModel):
    """oracle.plan_model.PlanModel with section 3y: the call is an export of tracers th and tq of the block, the operator and
    an import of tn and tt.  The block rule: only instances [sl0, sl0 + n) and tracers tn and tt change.  The error order:
    the block (n, sl0), the handle, the range, th / tq / tn, tt, two equal, the NULL pres, the NULL par, maxit, tol, the ramp
    with ICE, the mode, the precision of a host form, the state.  The interior-only rule: halo columns are neither read nor
    written.  The periodic rule: no wrap is part of the call and the plan clears its halo marks of tn and tt; every
    read-back and run of the model wraps again, as the plan does with cleared marks.  The windowed rule (that of 3t): the
    plan reads and writes owned levels only and clears the seam marks of tn and tt; the model holds the tall column, which
    is what the owners hold.  The marks of th and tq do not change: the model has none to change."""
    multi = False

    def satadj(self, th, tq, tn, tt, pres, gz=None, par=PAR, mode=0, sl0=0, n=None, eb=None):
        """-> (ncld, iters), each (n, nzm), or the code"""
        ncrms, nx, nz, T = self.dims
        n = ncrms - sl0 if n is None else n
        if n < 1 or sl0 < 0:
            return EINVAL
        if self.multi:
            return EUNSUPPORTED
        if sl0 + n > ncrms:
            return EINVAL
        if not (0 <= th < T and 0 <= tq < T and 0 <= tn < T) or not -1 <= tt < T:
            return EINVAL
        if len({th, tq, tn, tt}) != 4:
            return EINVAL
        if pres is None or par is None:
            return EINVAL
        if not 1 <= par["maxit"] <= 32 or not par["tol"] >= 0:
            return EINVAL
        if (mode & ICE) and not par["tmax"] > par["tmin"]:
            return EINVAL
        if mode & ~ICE:
            return EINVAL
        if eb is not None and eb != np.dtype(self.dtype).itemsize:
            return ESTATE
        if not self.uploaded:
            return ESTATE
        new, ncld, iters = satadj(self.a["f"][sl0:sl0 + n], th, tq, tn, tt, pres, gz, par, bool(mode & ICE))
        self.a["f"][sl0:sl0 + n] = new
        self._note()
        return ncld, iters
