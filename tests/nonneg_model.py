"""The model of the conservative per-level non-negativity fixer (include/mpdata_hip.h 3x) in plain numpy, the inputs its
tests share, and the plan model with the new call.

nonneg(f): the array of ONE block in the reference layout, f (n, nx+6, nzm[, T]) -> (f_new, sum (n, nzm[, T]), nneg (n,
nzm[, T])).  Every statement below is one elementwise operation on arrays of f's dtype, hence one rounding per element, in
the definition's association: s, p and c are explicit loops over i = 1 .. nx from +0 -- s = s + x; y = where(x > 0, x, +0);
p = p + y; c = c + where(x < 0, 1, 0) --, r = s / p ONE numpy division in f's dtype (numpy's division is the IEEE one), and
the new cell y * r.  Rows with c == 0 are copied, not computed; rows with c > 0 whose s is not positive become +0.  Only the
interior columns 1 .. nx (array index 3 .. nx+2) of f_new differ from f; halo columns are not read.

A row (instance, level, tracer) is a KEEP row (c == 0), a FIX row (c > 0 and s > 0) or a ZERO row (c > 0, s <= 0): kinds(f).
"""
import numpy as np

from oracle.plan_model import EINVAL, ESTATE, EUNSUPPORTED, PlanModel
from util import bits

KEEP, FIX, ZERO = 0, 1, 2


def _four(f):
    f = np.asarray(f)
    return f.reshape(f.shape + (1,)) if f.ndim == 3 else f


def reduce_rows(f):
    """-> (s, p, c), each (n, nzm, T), of f with a tracer axis"""
    n, nxp6, nzm, T = f.shape
    dt = f.dtype
    s, p, c = (np.zeros((n, nzm, T), dt) for _ in range(3))   # +0
    zero, one = dt.type(0), dt.type(1)
    for i in range(3, nxp6 - 3):
        x = f[:, i]
        s = s + x
        y = np.where(x > 0, x, zero)
        p = p + y
        c = c + np.where(x < 0, one, zero)
    for a in (s, p, c):
        assert a.dtype == dt
    return s, p, c


def nonneg(f):
    f = np.asarray(f)
    one_tracer = f.ndim == 3
    F = _four(f)
    dt = F.dtype
    nx = F.shape[1] - 6
    assert nx >= 1
    s, p, c = reduce_rows(F)
    ci = F[:, 3:nx + 3]                                     # columns 1 .. nx
    y = np.where(ci > 0, ci, dt.type(0))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = s / p                                           # one rounded division (used where c > 0 and s > 0 only)
        g = np.where((s > 0)[:, None], y * r[:, None], dt.type(0))   # s <= 0: +0 for every cell
    assert r.dtype == dt and y.dtype == dt and g.dtype == dt
    out = np.array(F, order="F")
    out[:, 3:nx + 3] = np.where((c > 0)[:, None], g, ci)    # c == 0: the row keeps every bit
    if one_tracer:
        out, s, c = out[..., 0], s[..., 0], c[..., 0]
    return np.asfortranarray(out), np.asfortranarray(s), np.asfortranarray(c)


def kinds(f):
    """(n, nzm, T) of KEEP / FIX / ZERO"""
    s, p, c = reduce_rows(_four(f))
    return np.where(c == 0, KEEP, np.where(s > 0, FIX, ZERO))


def has_all_kinds(f, sl0=0, n=None, first=0, ntr=None):
    """the block and tracer range of f holds keep rows and zero rows, and, where a row has more than one cell, fix rows
    (a row of one cell is kept or owes all it has)"""
    F = _four(f)
    n = F.shape[0] - sl0 if n is None else n
    ntr = F.shape[3] - first if ntr is None else ntr
    k = kinds(F[sl0:sl0 + n, ..., first:first + ntr])
    want = {KEEP, ZERO} | ({FIX} if F.shape[1] - 6 > 1 else set())
    return want <= set(np.unique(k).tolist())


def factors(f):
    """r (n, nzm, T) of the FIX rows of f, NaN elsewhere"""
    s, p, c = reduce_rows(_four(f))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = s / p
    return np.where((c > 0) & (s > 0), r, np.nan)


# ---- inputs.  uniform(-0.15, 1) in every cell, halo columns included (a walk that strays into a halo column meets other
# values, negative ones among them), and on five of every seven levels of an (instance, tracer) column a planted row:
#   0  wholly non-negative, one cell -0.0                    a KEEP row whose -0.0 must stay
#   1  wholly negative                                       a ZERO row
#   2  shifted by -0.6: mixed signs, s <= 0 for most         a ZERO row for most
#   3  scaled by 1e-3, one cell -1e-9                        a FIX row with r next to 1 (r == 1 in fp32 for some)
#   4  wholly non-negative with exact zeros                  a KEEP row
# the other two stay as drawn: FIX rows for most.  The pattern is shifted by instance and tracer, so every level meets
# every kind.
def make_field(n, nx, nz, T=None, dtype=np.float64, seed=0):
    """f (n, nx+6, nzm[, T]), Fortran order; T None: one tracer without the axis"""
    rng = np.random.default_rng([seed, n, nx, nz, 0 if T is None else T, 3])
    nzm, Tn = nz - 1, 1 if T is None else T
    f = rng.uniform(-0.15, 1.0, (n, nx + 6, nzm, Tn))
    col = rng.integers(0, nx, (n, nzm, Tn))                  # the planted cell of a row
    for b in range(n):
        for t in range(Tn):
            for k in range(nzm):
                kind = (k + b + 2 * t) % 7
                row = f[b, 3:nx + 3, k, t]
                j = col[b, k, t]
                if kind == 0:
                    row[:] = np.abs(row)
                    row[j] = -0.0
                elif kind == 1:
                    row[:] = -np.abs(row) - 1e-3
                elif kind == 2:
                    row[:] = row - 0.6
                elif kind == 3:
                    row[:] = np.abs(row) * 1e-3
                    row[j] = -1e-9
                elif kind == 4:
                    row[:] = np.abs(row)
                    row[j] = 0.0
                    row[(j + 1) % nx] = 0.0
    f = f.astype(dtype)
    return np.asfortranarray(f[..., 0] if T is None else f)


def make_clean_field(n, nx, nz, T=None, dtype=np.float64, seed=0):
    """a field without a negative cell in the interior: |make_field|, with its -0.0 and exact zeros kept as they are"""
    f = make_field(n, nx, nz, T, dtype, seed)
    neg = f < 0
    f[neg] = -f[neg]
    return f


def make_plan_inputs(oracle, shape, T=1, dtype=np.float64, seed=100):
    """the seven arrays of a plan, as subside_model.make_plan_inputs makes them (rho and adz in [0.5, 1); f and flux carry
    a tracer axis only for T > 1), with f from make_field"""
    import subside_model
    inp = subside_model.make_plan_inputs(oracle, shape, T, dtype, seed)
    f = make_field(*shape, None if T == 1 else T, dtype, seed)
    assert f.shape == inp["f"].shape and f.dtype == inp["f"].dtype
    inp["f"] = f
    return inp


class PlanModelNonneg(PlanModel):
    """oracle.plan_model.PlanModel with section 3x.  The block rule: only instances [sl0, sl0 + n) and tracers [first,
    first + ntr) change.  The error order: the block, the handle, the range, the tracers, the precision of a host form,
    the state (the call has no required array).  The interior-only rule: halo columns are neither read nor written -- the
    sums are those of the interior.  The periodic rule: no wrap is part of the call and the plan clears its halo marks;
    the halos a PERIODIC model then holds are those of the OLD field, and every read-back and run of the model wraps
    again, as the plan does with cleared marks.  The windowed rule (3r's): the plan reads and writes owned levels only and
    clears the seam marks of the range, so its next run refreshes every other copy from the owners; the model holds the
    tall column, which is what the owners hold."""
    multi = False

    def nonneg(self, sl0=0, n=None, first=0, ntr=None, eb=None):
        """-> (sum, nneg) with a tracer axis, or the code"""
        ncrms, nx, nz, T = self.dims
        n = ncrms - sl0 if n is None else n
        ntr = T - first if ntr is None else ntr
        if n < 1 or sl0 < 0:
            return EINVAL
        if self.multi:
            return EUNSUPPORTED
        if sl0 + n > ncrms or not self._tracers_ok(first, ntr):
            return EINVAL
        if eb is not None and eb != np.dtype(self.dtype).itemsize:
            return ESTATE
        if not self.uploaded:
            return ESTATE
        new, s, c = nonneg(self.a["f"][sl0:sl0 + n, ..., first:first + ntr])
        self.a["f"][sl0:sl0 + n, ..., first:first + ntr] = new
        self._note()
        return s, c
