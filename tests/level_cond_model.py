"""The model of the per-level conditional counts and sums (include/mpdata_hip.h 3v) in plain numpy, the variants its tests
hold it against, the inputs the tests share, and the plan model with the new call.

level_cond(F, tc, lo, hi, first, ntr): the arrays of ONE block in the reference layout -- F (n, nx+6, nzm, T), lo, hi (n,
nzm) or None -- -> (cnt (n, nzm), csum (n, nzm, ntr)); ntr = 0: csum is None.  It loops over the columns i = 1 .. nx in
order; every statement is one elementwise operation on arrays of F's dtype over (n, nzm), hence one rounding per element;
a column that is not in is SELECTED away (np.where), so what an excluded cell of a value tracer holds never reaches a sum.
Only the interior columns 1 .. nx (array index 3 .. nx+2) of tracer tc and the value tracers are read.  level_cond_loops
is the same as a plain-Python triple loop.

The variants (same signature, another arithmetic; none of them is the definition), by keyword: ge=True takes >= for >,
lt=True takes < for <=, reverse=True walks the columns from nx down to 1, multiply=True adds v_i times a 0 / 1 mask, shift=
True uses lo of level k - 1 (level 1: of the last level).
"""
import numpy as np

from oracle.plan_model import EINVAL, ESTATE, EUNSUPPORTED, PlanModel

VARIANTS = ("ge", "lt", "reverse", "multiply", "shift")


def level_cond(F, tc, lo=None, hi=None, first=0, ntr=None, ge=False, lt=False, reverse=False, multiply=False, shift=False):
    F = np.asarray(F)
    dt = F.dtype
    assert F.ndim == 4 and (lo is not None or hi is not None)
    n, nxp6, nzm, T = F.shape
    nx = nxp6 - 6
    ntr = T - first if ntr is None else ntr
    assert 0 <= tc < T and (ntr == 0 or (0 <= first and first + ntr <= T))
    for g in (lo, hi):
        assert g is None or (np.asarray(g).dtype == dt and np.asarray(g).shape == (n, nzm)), (dt, n, nzm)
    lo = None if lo is None else np.asarray(lo)
    hi = None if hi is None else np.asarray(hi)
    if shift and lo is not None:
        lo = np.roll(lo, 1, axis=1)
    one = dt.type(1)
    q = np.zeros((n, nzm), dt)                               # +0
    s = np.zeros((n, nzm, ntr), dt)                          # +0
    with np.errstate(invalid="ignore", over="ignore"):
        for i in (range(nx + 2, 2, -1) if reverse else range(3, nx + 3)):
            c = F[:, i, :, tc]
            inn = np.ones((n, nzm), bool)
            if lo is not None:
                inn &= (c >= lo) if ge else (c > lo)
            if hi is not None:
                inn &= (c < hi) if lt else (c <= hi)
            q = np.where(inn, q + one, q)
            v = F[:, i, :, first:first + ntr]
            if multiply:
                s = s + v * inn[..., None].astype(dt)
            else:
                s = np.where(inn[..., None], s + v, s)
    assert q.dtype == dt and s.dtype == dt
    return np.asfortranarray(q), (np.asfortranarray(s) if ntr else None)


def level_cond_loops(F, tc, lo=None, hi=None, first=0, ntr=None):
    """the definition as a plain triple loop over (instance, level, column), one rounded operation per statement"""
    F = np.asarray(F)
    R = F.dtype.type
    n, nxp6, nzm, T = F.shape
    nx = nxp6 - 6
    ntr = T - first if ntr is None else ntr
    cnt = np.zeros((n, nzm), F.dtype, order="F")
    csum = np.zeros((n, nzm, ntr), F.dtype, order="F")
    for b in range(n):
        for k in range(nzm):
            q, s = R(0), [R(0)] * ntr
            for i in range(3, nx + 3):
                c = F[b, i, k, tc]
                if (lo is None or c > lo[b, k]) and (hi is None or c <= hi[b, k]):
                    q = R(q + R(1))
                    for j in range(ntr):
                        s[j] = R(s[j] + F[b, i, k, first + j])
            cnt[b, k] = q
            csum[b, k] = s
    return cnt, (csum if ntr else None)


# ---- inputs.  f: the oracle's raw field moved by one half (subside_model.make_plan_inputs), so the sums take both signs,
# with column i (array index) scaled by COLUMN_SCALE[i mod 4].  The raw values are multiples of 2^-53 below one half, so
# every partial sum of a few of them is exact in fp64 and ANY order of the columns gives the same bits: a kernel that walks
# the columns backwards could not be told from the definition.  The factors are no powers of two, so the scaled values
# have full mantissas, the sums round and their order shows (tests/test_level_cond_cpu.py asserts how often).
COLUMN_SCALE = (1.0, 1.1, 0.9, 1.3)


def make_plan_inputs(oracle, shape, T=3, dtype=np.float64, seed=100):
    import subside_model
    inp = subside_model.make_plan_inputs(oracle, shape, T, dtype, seed)
    f = np.array(inp["f"], order="F")
    for i in range(f.shape[1]):
        f[:, i] *= np.dtype(dtype).type(COLUMN_SCALE[i % 4])
    inp["f"] = f
    return inp


BOUNDS = ("both", "lo", "hi")


def call_args(F, tc, bounds, seed):
    """(lo, hi) of a call on the block whose field is F (n, nx+6, nzm, T), each (n, nzm) in Fortran order or None; bounds:
    a name of BOUNDS.  Per row (b, k) two different interior columns of tracer tc are drawn; lo is the smaller of their two
    values and hi the larger, so that the ties c_i == lo (out) and c_i == hi (in) exist in every row.  Of every five
    levels, by (b + k) mod 5: one is EMPTY (0: lo >= hi -- the two values swapped, or lo = hi on every other such row; lo
    alone: the row's maximum; hi alone: below the row's minimum) and one holds EVERY column (1: lo below the row's minimum,
    hi the row's maximum).  nx = 3 and 4: THREE of five hold every column (1, 2, 3) -- another row has at most two columns
    in, whose sum has no order, and one row in five whose three terms round differently a quarter of the time cannot show
    a reversed walk in one output in ten.  nx = 1: the one column is both."""
    F = np.asarray(F)
    dt = F.dtype
    n, nxp6, nzm, T = F.shape
    nx = nxp6 - 6
    rng = np.random.default_rng([seed, n, nx, nzm, tc])
    c = F[:, 3:nx + 3, :, tc]                                # (n, nx, nzm)
    i1 = rng.integers(0, nx, (n, nzm))
    i2 = (i1 + rng.integers(1, max(nx, 2), (n, nzm))) % nx   # another column (nx = 1: the same)
    b, k = np.indices((n, nzm))
    v1, v2 = c[b, i1, k], c[b, i2, k]
    small, large = np.minimum(v1, v2), np.maximum(v1, v2)
    cmin, cmax = c.min(axis=1), c.max(axis=1)
    below = cmin - dt.type(1)
    kind = (b + k) % 5
    if nx in (3, 4):
        kind = np.where((kind == 2) | (kind == 3), 1, kind)
    if bounds == "both":
        lo = np.where(kind == 0, np.where((b + k) % 10 == 0, large, small), np.where(kind == 1, below, small))
        hi = np.where(kind == 0, small, np.where(kind == 1, cmax, large))
    elif bounds == "lo":
        lo, hi = np.where(kind == 0, cmax, np.where(kind == 1, below, v1)), None
    else:
        assert bounds == "hi"
        lo, hi = None, np.where(kind == 0, below, np.where(kind == 1, cmax, v1))
    F_ = lambda x: None if x is None else np.asfortranarray(x.astype(dt))
    return F_(lo), F_(hi)


def plant(F, tc, lo, hi, t):
    """a copy of F with +inf and NaN, in turn, in every cell of VALUE tracer t (not tc) whose column is not in"""
    F = np.array(F, order="F")
    assert t != tc
    n, nxp6, nzm, T = F.shape
    nx = nxp6 - 6
    c = F[:, 3:nx + 3, :, tc]
    inn = np.ones(c.shape, bool)
    if lo is not None:
        inn &= c > np.asarray(lo)[:, None]
    if hi is not None:
        inn &= c <= np.asarray(hi)[:, None]
    poison = np.where(np.indices(c.shape).sum(axis=0) % 2 == 0, np.inf, np.nan).astype(F.dtype)
    v = F[:, 3:nx + 3, :, t]
    F[:, 3:nx + 3, :, t] = np.where(inn, v, poison)
    return F


def share_differs(x, y):
    """the share of the elements of x and y that differ in bits"""
    from util import bits
    return float(np.mean(bits(np.asarray(x)) != bits(np.asarray(y))))


def variant_shares(F, triples, seed=7):
    """{variant: share of the outputs in which it differs from the definition}, over the (tc, first, ntr) triples with
    both bounds (shift: over cnt and csum of the calls; ge, lt: the same; reverse: csum alone -- a count has no order;
    multiply: csum of a planted value tracer, the variant against the definition on the same planted field)"""
    d = {v: [] for v in VARIANTS}
    for j, (tc, first, ntr) in enumerate(triples):
        lo, hi = call_args(F, tc, "both", seed + j)
        cnt, csum = level_cond(F, tc, lo, hi, first, ntr)
        for v in ("ge", "lt", "shift"):
            q, s = level_cond(F, tc, lo, hi, first, ntr, **{v: True})
            d[v].append((share_differs(cnt, q) + share_differs(csum, s)) / 2)
        d["reverse"].append(share_differs(csum, level_cond(F, tc, lo, hi, first, ntr, reverse=True)[1]))
        t = next(t for t in range(F.shape[3]) if t != tc)
        P = plant(F, tc, lo, hi, t)
        d["multiply"].append(share_differs(level_cond(P, tc, lo, hi, t, 1)[1], level_cond(P, tc, lo, hi, t, 1, multiply=True)[1]))
    return {k: float(np.mean(v)) for k, v in d.items()}


class PlanModelLevelCond(PlanModel):
    """oracle.plan_model.PlanModel with section 3v.  The call reads the interior columns of tracer tc and of the value
    tracers of instances [sl0, sl0 + n) and changes NOTHING of the model: no array, no flag, no bookkeeping.  The error
    order: the block (n, sl0), the handle, the range, tc, the two bounds, the two outputs, the tracer range where csum is
    asked for, the precision of a host form, the state.  Halo columns are not read, so the boundary mode has no face here;
    the model holds the tall column, which is what the owners of a windowed plan hold."""
    multi = False

    def level_cond(self, tc, lo=None, hi=None, first=0, ntr=None, sl0=0, n=None, eb=None, cnt=True, csum=True):
        """cnt, csum: whether the call passes the output -> (cnt or None, csum or None), or the code"""
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
        if not cnt and not csum:
            return EINVAL
        if csum and (first < 0 or ntr < 1 or first + ntr > T):
            return EINVAL
        if eb is not None and eb != np.dtype(self.dtype).itemsize:
            return ESTATE
        if not self.uploaded:
            return ESTATE
        q, s = level_cond(self.a["f"][sl0:sl0 + n], tc, lo, hi, first if csum else 0, ntr if csum else 0)
        return (q if cnt else None), s
