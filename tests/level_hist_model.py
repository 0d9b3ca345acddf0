"""The model of the per-level histograms (include/mpdata_hip.h 3ab) in plain numpy, the variants its tests hold it
against, the inputs the tests share, and the plan model with the new call.

level_hist(F, tc, edges, nb, first, ntr): the field of ONE block in the reference layout -- F (n, nx+6, nzm, T) --, edges a
sequence of at least nb + 1 doubles -> (cnt (n, nzm, nb), bsum (n, nzm, nb, ntr)); ntr = 0: bsum is None.  The edges are
rounded once to F's dtype.  It loops over the columns i = 1 .. nx in order; m_i is the number of the edges e_0 .. e_nb that
c_i exceeds, column i is in bin m_i - 1 where 1 <= m_i <= nb; every statement is one elementwise operation on arrays of F's
dtype, hence one rounding per element; a column outside a bin is SELECTED away (np.where), so what an excluded cell of a
value tracer holds never reaches a sum, and a NaN in c_i exceeds no edge and is in no bin.  Only the interior columns 1 ..
nx (array index 3 .. nx+2) of tracer tc and the value tracers are read.

The variants (same signature, another arithmetic; none of them is the definition), by keyword: ge=True takes >= for >,
off=True puts a column into bin m_i instead of m_i - 1, edge=True closes bin j at the edge of the wrong bin (e_{j+2} where
there is one), reverse=True walks the columns from nx down to 1, multiply=True adds v_i times a 0 / 1 mask, nan0=True counts
a NaN in bin 0.
"""
import numpy as np

from oracle.plan_model import EINVAL, ESTATE, EUNSUPPORTED, PlanModel

VARIANTS = ("ge", "off", "edge", "reverse", "multiply", "nan0")
MAX_BINS = 32


def level_hist(F, tc, edges, nb=None, first=0, ntr=None, ge=False, off=False, edge=False, reverse=False, multiply=False, nan0=False):
    F = np.asarray(F)
    dt = F.dtype
    assert F.ndim == 4
    n, nxp6, nzm, T = F.shape
    nx = nxp6 - 6
    nb = len(edges) - 1 if nb is None else nb
    ntr = T - first if ntr is None else ntr
    assert 0 <= tc < T and 1 <= nb <= MAX_BINS and (ntr == 0 or (0 <= first and first + ntr <= T))
    e = np.asarray(edges, np.float64)[:nb + 1].astype(dt)      # rounded once
    one = dt.type(1)
    q = np.zeros((n, nzm, nb), dt)                             # +0
    s = np.zeros((n, nzm, nb, ntr), dt)                        # +0
    jj = np.arange(nb)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in (range(nx + 2, 2, -1) if reverse else range(3, nx + 3)):
            c = F[:, i, :, tc]
            if edge:
                inn = (c[..., None] > e[jj]) & (c[..., None] <= e[np.minimum(jj + 2, nb)])
            else:
                m = ((c[..., None] >= e) if ge else (c[..., None] > e)).sum(axis=-1)       # 0 .. nb + 1
                if nan0:
                    m = np.where(np.isnan(c), 1, m)
                inn = (m[..., None] == jj) if off else (m[..., None] == jj + 1)             # (n, nzm, nb)
            q = np.where(inn, q + one, q)
            v = F[:, i, :, first:first + ntr][:, :, None, :]                                # (n, nzm, 1, ntr)
            if multiply:
                s = s + v * inn[..., None].astype(dt)
            else:
                s = np.where(inn[..., None], s + v, s)
    assert q.dtype == dt and s.dtype == dt
    return np.asfortranarray(q), (np.asfortranarray(s) if ntr else None)


# ---- inputs.  f: level_cond_model's field (both signs, full mantissas, columns scaled so that the order of a sum shows),
# stretched to about [-1, 2]; every fourth cell -- (i + 2 k + t) mod 4 = 0 -- is then QUANTISED to a multiple of 1/8.  The edges of
# call_edges lie on multiples of 1/4 (1/8 above twelve bins), so c == e_j occurs in most rows: a kernel that takes >= for >
# moves those columns one bin down.  The cells that are not quantised keep the sums of the value tracers rounding.
def make_plan_inputs(oracle, shape, T=3, dtype=np.float64, seed=100):
    import level_cond_model as LC
    inp = LC.make_plan_inputs(oracle, shape, T, dtype, seed)
    dt = np.dtype(dtype).type
    f = np.array(inp["f"], order="F") * dt(3) + dt(0.5)
    b, i, k, t = np.indices(f.shape)
    q = np.round(f * dt(8)) / dt(8)
    q = np.where(q == 0, dt(0.125), q)      # (no zero of either sign: a run returns -0.0 with the other sign -- convert_model.py)
    inp["f"] = np.asfortranarray(np.where((i + 2 * k + t) % 4 == 0, q, f).astype(dtype))
    return inp


def call_edges(nb, k):
    """nb + 1 non-decreasing float64 edges of call number k on the grid of the quantised cells (exact in fp32): from about
    -1 to 2, the ends moving with k by quarters; above 24 bins neighbouring edges repeat (empty bins); k mod 4 = 1, 2, 3: the
    first edge -inf, the last +inf, both"""
    grid = 0.25 if nb <= 12 else 0.125
    a, b = -1 + 0.25 * (k % 3), 2 - 0.25 * ((k // 3) % 3)
    e = np.round((a + (b - a) * np.arange(nb + 1) / nb) / grid) * grid
    if k % 4 in (1, 3):
        e[0] = -np.inf
    if k % 4 in (2, 3):
        e[-1] = np.inf
    assert (np.diff(e) >= 0).all() and (e.astype(np.float32) == e).all()
    return e


def sample_edges(F, tc, nb, seed):
    """nb + 1 values of tracer tc drawn from the interior of the block's field F, sorted (as float64: exact): every edge
    ties with a cell of the field"""
    F = np.asarray(F)
    nx = F.shape[1] - 6
    c = F[:, 3:nx + 3, :, tc].ravel()
    c = c[np.isfinite(c)]
    rng = np.random.default_rng([seed, nb, tc, F.shape[0]])
    return np.sort(rng.choice(c, nb + 1).astype(np.float64))


def plant(F, tc, edges, nb, t):
    """a copy of F with +inf and NaN, in turn, in every cell of VALUE tracer t (not tc) whose column is in no bin"""
    F = np.array(F, order="F")
    assert t != tc
    nx = F.shape[1] - 6
    e = np.asarray(edges, np.float64)[:nb + 1].astype(F.dtype)
    c = F[:, 3:nx + 3, :, tc]
    inn = (c > e[0]) & (c <= e[nb])
    poison = np.where(np.indices(c.shape).sum(axis=0) % 2 == 0, np.inf, np.nan).astype(F.dtype)
    F[:, 3:nx + 3, :, t] = np.where(inn, F[:, 3:nx + 3, :, t], poison)
    return F


def plant_nan(F, tc):
    """a copy of F with a NaN in tracer tc in one interior column of every row with (b + k) mod 3 = 0"""
    F = np.array(F, order="F")
    n, nxp6, nzm, T = F.shape
    b, k = np.indices((n, nzm))
    col = 3 + (b + 2 * k) % (nxp6 - 6)
    sel = (b + k) % 3 == 0
    F[b[sel], col[sel], k[sel], tc] = np.nan
    return F


def share_differs(x, y):
    """the share of the ROWS (b, k) of x and y in which any element differs in bits"""
    from util import bits
    d = bits(np.asarray(x)) != bits(np.asarray(y))
    return float(np.mean(d.reshape(d.shape[0], d.shape[1], -1).any(axis=2)))


def variant_shares(F, triples, nbs, seed=7):
    """{variant: share of the output rows in which it differs from the definition}, averaged over the (tc, first, ntr)
    triples and the bin counts (ge, off, edge: over cnt; reverse: bsum alone -- a count has no order -- and with one and two
    bins that hold every column, as the GPU tests' calls with nb = 1 and 2 nearly do: a bin of two columns has no order
    either; multiply: bsum of a
    planted value tracer, the variant against the definition on the same planted field; nan0: cnt on a field with NaNs
    planted in tc)"""
    d = {v: [] for v in VARIANTS}
    for j, ((tc, first, ntr), nb) in enumerate((tr, nb) for tr in triples for nb in nbs):
        e = call_edges(nb, seed + j)
        cnt, bsum = level_hist(F, tc, e, nb, first, ntr)
        for v in ("ge", "off", "edge"):
            d[v].append(share_differs(cnt, level_hist(F, tc, e, nb, first, 0, **{v: True})[0]))
        for nr in (1, 2):                                       # (many columns in a bin: else a sum has no order)
            er = call_edges(nr, 3)
            d["reverse"].append(share_differs(level_hist(F, tc, er, nr, first, ntr)[1], level_hist(F, tc, er, nr, first, ntr, reverse=True)[1]))
        t = next(t for t in range(F.shape[3]) if t != tc)
        ef = np.clip(e, -0.5, 1.5)                              # (some columns in no bin)
        P = plant(F, tc, ef, nb, t)
        d["multiply"].append(share_differs(level_hist(P, tc, ef, nb, t, 1)[1], level_hist(P, tc, ef, nb, t, 1, multiply=True)[1]))
        N = plant_nan(F, tc)
        d["nan0"].append(share_differs(level_hist(N, tc, e, nb, 0, 0)[0], level_hist(N, tc, e, nb, 0, 0, nan0=True)[0]))
    return {k: float(np.mean(v)) for k, v in d.items()}


class PlanModelLevelHist(PlanModel):
    """oracle.plan_model.PlanModel with section 3ab.  The call reads the interior columns of tracer tc and of the value
    tracers of instances [sl0, sl0 + n) and changes NOTHING of the model: no array, no flag, no bookkeeping.  The error
    order: the block (n, sl0), the handle, the range, tc, nb, the edges (null, a NaN or a descent), the two outputs, the
    tracer range where bsum is asked for, the precision of a host form, the state."""
    multi = False

    def level_hist(self, tc, edges, nb=None, first=0, ntr=None, sl0=0, n=None, eb=None, cnt=True, bsum=True):
        """cnt, bsum: whether the call passes the output -> (cnt or None, bsum or None), or the code"""
        ncrms, nx, nz, T = self.dims
        n = ncrms - sl0 if n is None else n
        ntr = T - first if ntr is None else ntr
        nb = (len(edges) - 1 if edges is not None else 0) if nb is None else nb
        if n < 1 or sl0 < 0:
            return EINVAL
        if self.multi:
            return EUNSUPPORTED
        if sl0 + n > ncrms:
            return EINVAL
        if not 0 <= tc < T:
            return EINVAL
        if not 1 <= nb <= MAX_BINS:
            return EINVAL
        if edges is None:
            return EINVAL
        e = np.asarray(edges, np.float64)[:nb + 1]
        if np.isnan(e).any() or (np.diff(e) < 0).any():
            return EINVAL
        if not cnt and not bsum:
            return EINVAL
        if bsum and (first < 0 or ntr < 1 or first + ntr > T):
            return EINVAL
        if eb is not None and eb != np.dtype(self.dtype).itemsize:
            return ESTATE
        if not self.uploaded:
            return ESTATE
        q, s = level_hist(self.a["f"][sl0:sl0 + n], tc, e, nb, first if bsum else 0, ntr if bsum else 0)
        return (q if cnt else None), s
