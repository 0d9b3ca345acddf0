"""The model of the per-level updraft / downdraft sampling (include/mpdata_hip.h 3ac) in plain numpy, the variants its tests
hold it against, the inputs the tests share, and the plan model with the new call.

level_draft(F, W, tc, lo, hi, wup, wdn, first, ntr): the fields of ONE block in the reference layout -- F (n, nx+6, nzm, T),
W (n, nx+4, nz) -- -> (cnt (n, nzm, 3), wsum (n, nzm, 3), fsum (n, nzm, 3, ntr), wfsum (n, nzm, 3, ntr)); ntr = 0: fsum and
wfsum are None.  tc = -1: no tracer condition (lo and hi None).  The thresholds are rounded once to W's dtype.  It loops over
the columns i = 1 .. nx in order; every statement is one elementwise operation on arrays of the fields' dtype, hence one
rounding per element: a = w(k) + wk1 (wk1 = +0 at the top level: W[:, :, nz-1] is never read), wc = 0.5 * a, p = wc * v.  A
column outside a class is SELECTED away (np.where), so what an excluded cell of a value tracer holds never reaches a sum.
Only the interior columns 1 .. nx of W (array index 2 .. nx+1), of tracer tc and of the value tracers (3 .. nx+2) are read.

The variants (same signature, another arithmetic; none of them is the definition), by keyword: ge=True takes >= for > and <=
for < in the class tests, swap=True exchanges UP and DOWN, below=True takes w(k) for wk1, top_read=True reads W[:, :, nz-1] at
the top level, wsum_v=True forms wfsum as wsum-style sum of wc times the class sum of v (the product of the sums), multiply=
True adds values times a 0 / 1 mask, reverse=True walks the columns from nx down to 1.
"""
import numpy as np

from oracle.plan_model import EINVAL, ESTATE, EUNSUPPORTED, PlanModel

VARIANTS = ("ge", "swap", "below", "top_read", "wsum_v", "multiply", "reverse")
UP, DOWN, ENV = 0, 1, 2
WUP, WDN = 0.25, -0.25


def level_draft(F, W, tc=-1, lo=None, hi=None, wup=WUP, wdn=WDN, first=0, ntr=None, ge=False, swap=False, below=False,
                top_read=False, wsum_v=False, multiply=False, reverse=False):
    W = np.asarray(W)
    dt = W.dtype
    n, nxp4, nz = W.shape
    nx, nzm = nxp4 - 4, nz - 1
    if F is None:
        assert tc < 0 and ntr == 0
        T = 0
    else:
        F = np.asarray(F)
        assert F.ndim == 4 and F.dtype == dt and F.shape[:3] == (n, nx + 6, nzm), (F.shape, W.shape)
        T = F.shape[3]
    ntr = T - first if ntr is None else ntr
    assert -1 <= tc < max(T, 1) and (ntr == 0 or (0 <= first and first + ntr <= T))
    assert tc >= 0 or (lo is None and hi is None)
    for g in (lo, hi):
        assert g is None or (np.asarray(g).dtype == dt and np.asarray(g).shape == (n, nzm)), (dt, n, nzm)
    lo = None if lo is None else np.asarray(lo)
    hi = None if hi is None else np.asarray(hi)
    up_t, dn_t = np.asarray(wup, np.float64).astype(dt), np.asarray(wdn, np.float64).astype(dt)      # rounded once
    assert dn_t <= up_t
    half, one = dt.type(0.5), dt.type(1)
    zero = np.zeros((n, 1), dt)                              # +0
    q = np.zeros((n, nzm, 3), dt)
    sw = np.zeros((n, nzm, 3), dt)
    sf = np.zeros((n, nzm, 3, ntr), dt)
    swf = np.zeros((n, nzm, 3, ntr), dt)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in (range(nx, 0, -1) if reverse else range(1, nx + 1)):
            w0 = W[:, i + 1, :nzm]
            if below:
                wk1 = w0
            elif top_read:
                wk1 = W[:, i + 1, 1:nzm + 1]
            else:
                wk1 = np.concatenate([W[:, i + 1, 1:nzm], zero], axis=1)
            a = w0 + wk1
            wc = half * a
            inn = np.ones((n, nzm), bool)
            if tc >= 0:
                c = F[:, i + 2, :, tc]
                if lo is not None:
                    inn &= c > lo
                if hi is not None:
                    inn &= c <= hi
            up = (wc >= up_t) if ge else (wc > up_t)
            dn = ((wc <= dn_t) if ge else (wc < dn_t)) & ~up
            cls = np.stack([inn & up, inn & dn, inn & ~up & ~dn], axis=-1)                          # (n, nzm, 3)
            if swap:
                cls = cls[..., [1, 0, 2]]
            q = np.where(cls, q + one, q)
            sw = np.where(cls, sw + wc[..., None], sw)
            if ntr:
                v = F[:, i + 2, :, first:first + ntr][:, :, None, :]                                # (n, nzm, 1, ntr)
                p = wc[:, :, None, None] * v
                if multiply:
                    m = cls[..., None].astype(dt)
                    sf = sf + v * m
                    swf = swf + p * m
                else:
                    sf = np.where(cls[..., None], sf + v, sf)
                    swf = np.where(cls[..., None], swf + p, swf)
        if wsum_v and ntr:
            swf = sw[..., None] * sf
    assert q.dtype == dt and sw.dtype == dt and sf.dtype == dt and swf.dtype == dt
    A = np.asfortranarray
    return A(q), A(sw), (A(sf) if ntr else None), (A(swf) if ntr else None)


def level_draft_loops(F, W, tc=-1, lo=None, hi=None, wup=WUP, wdn=WDN, first=0, ntr=None):
    """the definition as a plain triple loop over (instance, level, column), one rounded operation per statement"""
    W = np.asarray(W)
    R = W.dtype.type
    n, nxp4, nz = W.shape
    nx, nzm = nxp4 - 4, nz - 1
    T = 0 if F is None else F.shape[3]
    ntr = T - first if ntr is None else ntr
    wu, wd = R(np.float64(wup)), R(np.float64(wdn))
    cnt = np.zeros((n, nzm, 3), W.dtype, order="F")
    wsum = np.zeros((n, nzm, 3), W.dtype, order="F")
    fsum = np.zeros((n, nzm, 3, ntr), W.dtype, order="F")
    wfsum = np.zeros((n, nzm, 3, ntr), W.dtype, order="F")
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(n):
            for k in range(nzm):
                for i in range(1, nx + 1):
                    wk1 = W[b, i + 1, k + 1] if k + 1 < nzm else R(0)
                    a = R(W[b, i + 1, k] + wk1)
                    wc = R(R(0.5) * a)
                    if tc >= 0:
                        c = F[b, i + 2, k, tc]
                        if not ((lo is None or c > lo[b, k]) and (hi is None or c <= hi[b, k])):
                            continue
                    cl = UP if wc > wu else DOWN if wc < wd else ENV
                    cnt[b, k, cl] = R(cnt[b, k, cl] + R(1))
                    wsum[b, k, cl] = R(wsum[b, k, cl] + wc)
                    for j in range(ntr):
                        v = F[b, i + 2, k, first + j]
                        fsum[b, k, cl, j] = R(fsum[b, k, cl, j] + v)
                        p = R(wc * v)
                        wfsum[b, k, cl, j] = R(wfsum[b, k, cl, j] + p)
    return cnt, wsum, (fsum if ntr else None), (wfsum if ntr else None)


# ---- inputs.  f: level_cond_model's field (both signs, full mantissas, columns scaled so that the order of a sum shows).
# w: from the oracle's raw signed r in [-0.5, 0.5) (multiples of 2^-53: every partial sum of them is exact in fp64 and no
# order would show), w = sign(r) * 0.5 * sqrt(2 |r|): full mantissas, still inside [-0.5, 0.5] as the velocities of every
# other test, but with more weight towards the ends, so that about one cell-centred wc in five lies above 0.25 and one in
# five below -0.25 (of r itself: one in ten) and the draft classes are not nearly empty at nx = 2 and 3.  Every fourth value
# -- (i + k) mod 4 = 0 over the array indices -- is then QUANTISED to a multiple of 1/8.  The default thresholds WUP = 0.25
# and WDN = -0.25 sit on that grid.  wc is the mean of TWO levels, of which at most one is quantised in a column, so the grid
# alone makes a tie only at the top level (wk1 = +0 there); plant_ties therefore sets, in every row (b, k), one interior
# column to wc == WUP and another to wc == WDN exactly (both levels of the pair equal to the threshold, the columns moving by
# two per level so that the rows do not collide).  So wc == wup and wc == wdn occur in most rows, and a kernel that takes >=
# for > moves those columns from ENV to a draft.  A level then holds four planted columns, so nx < 8 has no room for that:
# there every FOURTH row is planted, so that the other rows keep columns outside ENV.  w(:, :, nz) is filled with nonzero values up to 2 in size (the recipe of
# tests/courant_model.py), so a read of it shows.
def make_plan_inputs(oracle, shape, T=3, dtype=np.float64, seed=100):
    import level_cond_model as LC
    inp = LC.make_plan_inputs(oracle, shape, T, dtype, seed)
    dt = np.dtype(dtype).type
    r = np.array(inp["w"], order="F")
    w = (np.sign(r) * dt(0.5) * np.sqrt(dt(2) * np.abs(r))).astype(dtype)
    n, nxp4, nz = w.shape
    b, i, k = np.indices(w.shape)
    q = np.round(w * dt(8)) / dt(8)
    q = np.where(q == 0, dt(0.125), q)       # (no zero of either sign; the -0.0 rule has its own test)
    w = np.where((i + k) % 4 == 0, q, w).astype(dtype)
    w = plant_ties(w, WUP, WDN)
    top = oracle.make_inputs(*shape, seed=seed + 1000, dist=oracle.DIST_RAW_SIGNED, dtype=dtype)["w"][:, :, 0]
    w[:, :, nz - 1] = np.where(top == 0, dt(0.25), top) * dt(4)
    inp["w"] = np.asfortranarray(w)
    assert inp["w"].dtype == np.dtype(dtype) and inp["f"].dtype == np.dtype(dtype) and np.all(inp["w"][:, :, -1] != 0)
    return inp


def plant_ties(w, wup, wdn):
    """a copy of w in which row (b, k) has wc == wup in interior column 1 + (b + 2 k) mod nx and wc == wdn in column 1 + (b + 2
    k + 1) mod nx (nx = 1: the first alone): both levels k and k + 1 of the column are set to the threshold, at the top level
    (wk1 = +0) level k to twice the threshold.  nx < 8: only the rows with k a multiple of four.  Finite thresholds; exact in
    fp32 where 2 * threshold is."""
    w = np.array(w, order="F")
    n, nxp4, nz = w.shape
    nx, nzm = nxp4 - 4, nz - 1
    dt = w.dtype.type
    for b in range(n):
        for k in range(0, nzm, 1 if nx >= 8 else 4):
            cols = ((1 + (b + 2 * k) % nx, wup), (1 + (b + 2 * k + 1) % nx, wdn))
            for i, t in cols[:min(nx, 2)]:
                if k + 1 < nzm:
                    w[b, i + 1, k] = dt(t)
                    w[b, i + 1, k + 1] = dt(t)
                else:
                    w[b, i + 1, k] = dt(2 * t)
    return w


def tie_share(W, wup, wdn):
    """the shares of the rows (b, k) of W that hold a column with wc == wup and with wc == wdn"""
    W = np.asarray(W)
    n, nxp4, nz = W.shape
    nx, nzm = nxp4 - 4, nz - 1
    wk1 = np.concatenate([W[:, 2:nx + 2, 1:nzm], np.zeros((n, nx, 1), W.dtype)], axis=2)
    wc = W.dtype.type(0.5) * (W[:, 2:nx + 2, :nzm] + wk1)
    return float(np.mean((wc == W.dtype.type(wup)).any(axis=1))), float(np.mean((wc == W.dtype.type(wdn)).any(axis=1)))


THRESHOLDS = ((WUP, WDN), (WUP, -np.inf), (np.inf, WDN), (np.inf, -np.inf), (WUP, WUP), (WDN, WDN))
"""the threshold pairs the tests rotate through: on the grid, one-sided infinite (twice), both infinite, wdn == wup (twice)"""


def plant(F, W, tc, lo, hi, wup, wdn, t, cls):
    """a copy of F with +inf and NaN, in turn, in every cell of VALUE tracer t (not tc) whose column is NOT in class cls"""
    F = np.array(F, order="F")
    assert t != tc
    W = np.asarray(W)
    n, nxp4, nz = W.shape
    nx, nzm = nxp4 - 4, nz - 1
    dt = W.dtype
    wk1 = np.concatenate([W[:, 2:nx + 2, 1:nzm], np.zeros((n, nx, 1), dt)], axis=2)
    wc = dt.type(0.5) * (W[:, 2:nx + 2, :nzm] + wk1)
    inn = np.ones(wc.shape, bool)
    if tc >= 0:
        c = F[:, 3:nx + 3, :, tc]
        if lo is not None:
            inn &= c > np.asarray(lo)[:, None]
        if hi is not None:
            inn &= c <= np.asarray(hi)[:, None]
    up, dn = wc > dt.type(wup), wc < dt.type(wdn)
    member = inn & (up if cls == UP else dn if cls == DOWN else ~up & ~dn)
    poison = np.where(np.indices(wc.shape).sum(axis=0) % 2 == 0, np.inf, np.nan).astype(dt)
    F[:, 3:nx + 3, :, t] = np.where(member, F[:, 3:nx + 3, :, t], poison)
    return F


def share_differs(xs, ys):
    """the share of the ROWS (b, k) in which any element of any of the paired arrays differs in bits (None pairs skipped)"""
    from util import bits
    d = None
    for x, y in zip(xs, ys):
        if x is None:
            continue
        e = bits(np.asarray(x)) != bits(np.asarray(y))
        e = e.reshape(e.shape[0], e.shape[1], -1).any(axis=2)
        d = e if d is None else d | e
    return float(np.mean(d))


def variant_share(name, F, W, tc, lo, hi, wup, wdn, first, ntr):
    """the share of the output rows in which variant `name` differs from the definition on this call (reverse: over the sums
    alone -- a count has no order; wsum_v: over wfsum; multiply: over fsum and wfsum of a planted value tracer against the
    definition on the same planted field, the ENV class kept)"""
    if name == "multiply":
        t = next(t for t in range(F.shape[3]) if t != tc)
        P = plant(F, W, tc, lo, hi, wup, wdn, t, ENV)
        ref = level_draft(P, W, tc, lo, hi, wup, wdn, t, 1)
        var = level_draft(P, W, tc, lo, hi, wup, wdn, t, 1, multiply=True)
        return share_differs(ref[2:], var[2:])
    ref = level_draft(F, W, tc, lo, hi, wup, wdn, first, ntr)
    var = level_draft(F, W, tc, lo, hi, wup, wdn, first, ntr, **{name: True})
    if name == "reverse":
        return share_differs(ref[1:], var[1:])
    if name == "wsum_v":
        return share_differs(ref[3:], var[3:])
    return share_differs(ref, var)


class PlanModelLevelDraft(PlanModel):
    """oracle.plan_model.PlanModel with section 3ac.  The call reads the interior columns of w, of tracer tc and of the value
    tracers of instances [sl0, sl0 + n) and changes NOTHING of the model: no array, no flag, no bookkeeping.  The error
    order: the block (n, sl0), the handle, the range, tc, lo / hi without a condition tracer, the thresholds (a NaN, wdn >
    wup), the four outputs, the tracer range where fsum or wfsum is asked for, the precision of a host form, the state
    (never filled; w not held)."""
    multi = False

    def level_draft(self, tc=-1, lo=None, hi=None, wup=WUP, wdn=WDN, first=0, ntr=None, sl0=0, n=None, eb=None, cnt=True, wsum=True,
                    fsum=True, wfsum=True):
        """cnt .. wfsum: whether the call passes the output -> the four outputs (None where not passed), or the code"""
        ncrms, nx, nz, T = self.dims
        n = ncrms - sl0 if n is None else n
        ntr = T - first if ntr is None else ntr
        if n < 1 or sl0 < 0:
            return EINVAL
        if self.multi:
            return EUNSUPPORTED
        if sl0 + n > ncrms:
            return EINVAL
        if not -1 <= tc < T:
            return EINVAL
        if tc < 0 and (lo is not None or hi is not None):
            return EINVAL
        if np.isnan(wup) or np.isnan(wdn) or wdn > wup:
            return EINVAL
        if not (cnt or wsum or fsum or wfsum):
            return EINVAL
        sums = fsum or wfsum
        if sums and (first < 0 or ntr < 1 or first + ntr > T):
            return EINVAL
        if eb is not None and eb != np.dtype(self.dtype).itemsize:
            return ESTATE
        if not self.uploaded or not self.have_w:
            return ESTATE
        f = self.a["f"][sl0:sl0 + n]
        if f.ndim == 3:
            f = f[..., None]
        q, sw, sf, swf = level_draft(f, self.a["w"][sl0:sl0 + n], tc, lo, hi, wup, wdn, first if sums else 0, ntr if sums else 0)
        return (q if cnt else None), (sw if wsum else None), (sf if fsum else None), (swf if wfsum else None)
