"""The model of the per-column conditional level counts, tops and paths (include/mpdata_hip.h 3w) in plain numpy, the
variants its tests hold it against, the inputs the tests share, and the plan model with the new call.

column_cond(F, rho, adz, tc, lo, hi, first, ntr): the arrays of ONE block in the reference layout -- F (n, nx+6, nzm, T),
rho, adz (n, nzm), lo, hi (n, nzm) or None -- -> a dict of kcnt, kbot, ktop (n, nx), cpath (n, nx, ntr), cover (n,), mass
(n, ntr), Fortran order; ntr = 0: cpath and mass are None.  It loops over the levels k = 1 .. nzm in order; every statement
is one elementwise operation on arrays of F's dtype over (n, nx), hence one rounding per element; a level that is not in is
SELECTED away (np.where), so what an excluded cell of a value tracer holds never reaches a sum.  Only the interior columns
1 .. nx (array index 3 .. nx+2) of tracer tc and the value tracers are read.  column_cond_loops is the same as a
plain-Python triple loop.

The variants (same signature, another arithmetic; none of them is the definition), by keyword: ge=True takes >= for >,
lt=True takes < for <=, reverse=True walks the levels from nzm down to 1, multiply=True adds wgt * v times a 0 / 1 mask,
contract=True forms s + wgt * v exactly and rounds once (an fma), shift_lo=True uses lo of level k - 1 (level 1: of the
last level), shift_w=True the weight of level k - 1, swap=True exchanges ktop and kbot, local=nz writes the window-local
level index of a windowed plan of nz levels into ktop and kbot."""
from fractions import Fraction

import numpy as np

import level_cond_model as LC
import level_stats_model as LM
from column_path_model import _round_f32, mass_of
from oracle.plan_model import EINVAL, ESTATE, EUNSUPPORTED, PlanModel

VARIANTS = ("ge", "lt", "reverse", "multiply", "contract", "shift_lo", "shift_w", "swap")
OUTPUTS = ("kcnt", "kbot", "ktop", "cpath", "cover", "mass")
BOUNDS = LC.BOUNDS


def level_window(nz, h):
    """(W, k0, own0, own1) of window h of a column of nz levels (csrc/mpdata_windows.h), 1-based tall levels"""
    nzm = nz - 1
    W, m = 1, nzm
    if nz > 64:
        W = (nzm - 6 + 56) // 57
        m = (nzm + 6 * (W - 1) + W - 1) // W
    D = nzm - m
    a = h * D // (W - 1) if W > 1 else 0
    b = (h + 1) * D // (W - 1) if h + 1 < W else 0
    return W, a, (1 if h == 0 else a + 4), (nzm if h == W - 1 else b + 3)


def local_level(nz):
    """tall level k = 1 .. nzm -> the level index inside the window that owns it (array index k - 1)"""
    out = np.zeros(nz - 1, np.int64)
    W = level_window(nz, 0)[0]
    for h in range(W):
        _, k0, own0, own1 = level_window(nz, h)
        out[own0 - 1:own1] = np.arange(own0, own1 + 1) - k0
    return out


def _fma(s, w, v):
    """s + w * v formed exactly and rounded once to the dtype, elementwise"""
    dt = s.dtype
    out = np.empty(s.shape, dt)
    w = np.broadcast_to(w, s.shape)
    for ix in np.ndindex(s.shape):
        if not (np.isfinite(s[ix]) and np.isfinite(w[ix]) and np.isfinite(v[ix])):
            out[ix] = s[ix] + w[ix] * v[ix]
            continue
        x = Fraction(float(s[ix])) + Fraction(float(w[ix])) * Fraction(float(v[ix]))
        out[ix] = x.numerator / x.denominator if dt == np.float64 else _round_f32(x)
    return out


def column_cond(F, rho, adz, tc, lo=None, hi=None, first=0, ntr=None, ge=False, lt=False, reverse=False, multiply=False,
                contract=False, shift_lo=False, shift_w=False, swap=False, local=None):
    F, rho, adz = np.asarray(F), np.asarray(rho), np.asarray(adz)
    dt = F.dtype
    assert F.ndim == 4 and (lo is not None or hi is not None)
    n, nxp6, nzm, T = F.shape
    nx = nxp6 - 6
    ntr = T - first if ntr is None else ntr
    assert 0 <= tc < T and (ntr == 0 or (0 <= first and first + ntr <= T))
    for g in (lo, hi, rho, adz):
        assert g is None or (np.asarray(g).dtype == dt and np.asarray(g).shape == (n, nzm)), (dt, n, nzm)
    lo = None if lo is None else np.asarray(lo)
    hi = None if hi is None else np.asarray(hi)
    wgt = rho * adz                                          # one rounded multiply
    assert wgt.dtype == dt
    if shift_lo and lo is not None:
        lo = np.roll(lo, 1, axis=1)
    if shift_w:
        wgt = np.roll(wgt, 1, axis=1)
    lev = np.arange(1, nzm + 1) if local is None else local_level(local)
    assert len(lev) == nzm
    one = dt.type(1)
    q = np.zeros((n, nx), dt)                                # +0
    bot = np.zeros((n, nx), dt)
    top = np.zeros((n, nx), dt)
    s = np.zeros((n, nx, ntr), dt)                           # +0
    with np.errstate(invalid="ignore", over="ignore"):
        for k in (range(nzm - 1, -1, -1) if reverse else range(nzm)):
            c = F[:, 3:nx + 3, k, tc]
            inn = np.ones((n, nx), bool)
            if lo is not None:
                inn &= (c >= lo[:, None, k]) if ge else (c > lo[:, None, k])
            if hi is not None:
                inn &= (c < hi[:, None, k]) if lt else (c <= hi[:, None, k])
            q = np.where(inn, q + one, q)
            here = dt.type(lev[k])
            if reverse:                                      # (smallest and largest k: not a matter of the order)
                top = np.where(inn & (top == 0), here, top)
                bot = np.where(inn, here, bot)
            else:
                bot = np.where(inn & (bot == 0), here, bot)
                top = np.where(inn, here, top)
            if ntr:
                v = F[:, 3:nx + 3, k, first:first + ntr]
                w = wgt[:, None, k, None]
                if contract:
                    s = np.where(inn[..., None], _fma(s, w, v), s)
                elif multiply:
                    s = s + (w * v) * inn[..., None].astype(dt)
                else:
                    prod = w * v                             # rounded to the dtype
                    assert prod.dtype == dt
                    s = np.where(inn[..., None], s + prod, s)
    assert q.dtype == dt and s.dtype == dt and bot.dtype == dt and top.dtype == dt
    if swap:
        bot, top = top, bot
    cover = np.zeros((n,), dt)
    for i in range(nx):
        cover = np.where(q[:, i] > 0, cover + one, cover)
    A = np.asfortranarray
    return {"kcnt": A(q), "kbot": A(bot), "ktop": A(top), "cpath": A(s) if ntr else None, "cover": A(cover),
            "mass": mass_of(s) if ntr else None}


def column_cond_loops(F, rho, adz, tc, lo=None, hi=None, first=0, ntr=None):
    """the definition as a plain triple loop over (instance, column, level), one rounded operation per statement"""
    F = np.asarray(F)
    R = F.dtype.type
    n, nxp6, nzm, T = F.shape
    nx = nxp6 - 6
    ntr = T - first if ntr is None else ntr
    new = lambda *sh: np.zeros(sh, F.dtype, order="F")
    out = {"kcnt": new(n, nx), "kbot": new(n, nx), "ktop": new(n, nx), "cpath": new(n, nx, ntr), "cover": new(n), "mass": new(n, ntr)}
    for b in range(n):
        cov, mass = R(0), [R(0)] * ntr
        for i in range(3, nx + 3):
            q, bot, top, s = R(0), R(0), R(0), [R(0)] * ntr
            for k in range(nzm):
                c = F[b, i, k, tc]
                if (lo is None or c > lo[b, k]) and (hi is None or c <= hi[b, k]):
                    q = R(q + R(1))
                    if bot == 0:
                        bot = R(k + 1)
                    top = R(k + 1)
                    wgt = R(rho[b, k] * adz[b, k])
                    for j in range(ntr):
                        s[j] = R(s[j] + R(wgt * F[b, i, k, first + j]))
            out["kcnt"][b, i - 3], out["kbot"][b, i - 3], out["ktop"][b, i - 3] = q, bot, top
            out["cpath"][b, i - 3] = s
            if q > 0:
                cov = R(cov + R(1))
            mass = [R(mass[j] + s[j]) for j in range(ntr)]
        out["cover"][b] = cov
        out["mass"][b] = mass
    if not ntr:
        out["cpath"] = out["mass"] = None
    return out


# ---- inputs.  The fields: level_stats_model.make (raw signed magnitudes, column i scaled by 2**-(i mod 4)), as the column
# integrals of 3k take them; rho and adz are the ones it returns.  The bounds: level_cond_model.call_args -- lo and hi of a
# row (b, k) are values of two of its own columns, so the ties c == lo (out) and c == hi (in) exist; one level in five is
# empty and one in five is full.
def make_plan_inputs(oracle, shape, T=3, dtype=np.float64, seed=100):
    return LM.make(oracle, shape, T, dtype, seed)


call_args = LC.call_args


def all_in(F, tc):
    """hi alone, above every value of tracer tc: every level of every column is in"""
    F = np.asarray(F)
    return None, np.full((F.shape[0], F.shape[2]), np.inf, F.dtype, order="F")


def plant(F, tc, lo, hi, t):
    """a copy of F with +inf and NaN, in turn, in every cell of VALUE tracer t (not tc) whose level is not in"""
    return LC.plant(F, tc, lo, hi, t)


def differs(x, y):
    """whether any element of any output of the two results differs in bits"""
    from util import bits
    for k in OUTPUTS:
        if (x[k] is None) != (y[k] is None):
            return True
        if x[k] is not None and not np.array_equal(bits(np.asarray(x[k])), bits(np.asarray(y[k]))):
            return True
    return False


def variants_that_change(inp, triples, nz_windowed=None, seed=7, sub=2):
    """{variant: True where it changes at least one element of at least one output}, over the (tc, first, ntr) triples with
    both bounds on the inputs inp (f, rho, adz).  multiply: on a planted field.  contract: on the first `sub` instances and
    the first value tracer (the exact arithmetic is slow; an instance's outputs are functions of that instance alone).
    nz_windowed: the levels of a windowed shape -- then "local" is measured too."""
    F, rho, adz = inp["f"], inp["rho"], inp["adz"]
    names = VARIANTS + (("local",) if nz_windowed else ())
    d = dict.fromkeys(names, False)
    for j, (tc, first, ntr) in enumerate(triples):
        lo, hi = call_args(F, tc, "both", seed + j)
        base = column_cond(F, rho, adz, tc, lo, hi, first, ntr)
        for v in names:
            if d[v] or v in ("multiply", "contract"):
                continue
            kw = {v: True} if v != "local" else {"local": nz_windowed}
            d[v] = differs(base, column_cond(F, rho, adz, tc, lo, hi, first, ntr, **kw))
        if not d["multiply"]:
            t = next(t for t in range(F.shape[3]) if t != tc)
            P = plant(F, tc, lo, hi, t)
            d["multiply"] = differs(column_cond(P, rho, adz, tc, lo, hi, t, 1), column_cond(P, rho, adz, tc, lo, hi, t, 1, multiply=True))
        if not d["contract"]:
            b = slice(0, sub)
            args = (np.asfortranarray(F[b]), rho[b], adz[b], tc, lo[b], hi[b], first, 1)
            d["contract"] = differs(column_cond(*args), column_cond(*args, contract=True))
    return d


class PlanModelColumnCond(PlanModel):
    """oracle.plan_model.PlanModel with section 3w.  The call reads the interior columns of tracer tc and of the value
    tracers, rho and adz of instances [sl0, sl0 + n) and changes NOTHING of the model: no array, no flag, no bookkeeping.
    The error order: the block (n, sl0), the handle, the range, tc, the two bounds, the six outputs, cover without kcnt and
    mass without cpath, the tracer range where cpath is asked for, the precision of a host form, the state.  Halo columns
    are not read, so the boundary mode has no face here; the model holds the tall column, which is what the owners of a
    windowed plan hold."""
    multi = False

    def column_cond(self, tc, lo=None, hi=None, first=0, ntr=None, sl0=0, n=None, eb=None, outs=OUTPUTS):
        """outs: the names of the outputs the call passes -> {name: array} of those, or the code"""
        ncrms, nx, nz, T = self.dims
        n = ncrms - sl0 if n is None else n
        ntr = T - first if ntr is None else ntr
        if n < 1 or sl0 < 0:
            return EINVAL
        if self.multi:
            return EUNSUPPORTED
        if sl0 + n > ncrms:
            return EINVAL
        if not 0 <= tc < T:
            return EINVAL
        if lo is None and hi is None:
            return EINVAL
        if not outs:
            return EINVAL
        if ("cover" in outs and "kcnt" not in outs) or ("mass" in outs and "cpath" not in outs):
            return EINVAL
        if "cpath" in outs and (first < 0 or ntr < 1 or first + ntr > T):
            return EINVAL
        if eb is not None and eb != np.dtype(self.dtype).itemsize:
            return ESTATE
        if not self.uploaded:
            return ESTATE
        b = slice(sl0, sl0 + n)
        path = "cpath" in outs
        r = column_cond(self.a["f"][b], self.a["rho"][b], self.a["adz"][b], tc, lo, hi, first if path else 0, ntr if path else 0)
        return {k: r[k] for k in outs}
