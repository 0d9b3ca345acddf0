"""The model of the linear combinations of tracers (include/mpdata_hip.h 3z) in plain numpy, the inputs its tests share, and
the plan model with the new call.

combine(f, dst, src, coef, c0, clip): the arrays of ONE block in the reference layout -- f (n, nx+6, nzm, T), coef (n, nzm,
nsrc) or None, c0 (n, nzm) or None -- -> (f_new, sum (n, nzm)).  Every statement below is one elementwise operation on
arrays of f's dtype, hence one rounding per element, in the definition's association: the first source is taken (times its
coefficient), the others are added one by one in the order of src, c0 last; the clip is np.where on a plain `>`, so NaN and
-0 fall to the +0 branch; sum is an explicit loop over i = 1 .. nx from +0.  Without coef nothing is multiplied, so one
source without c0 and without the clip is a copy of bits.  Every source is read from f, the OLD field, also where it is
dst.  Only the interior columns 1 .. nx (array index 3 .. nx+2) of tracer dst of f_new differ from f; halo columns and
tracers that are no source are not read.  combine_loops is the same as a scalar triple loop, statement by statement.

NaN: IEEE 754 leaves the sign and payload of a NaN that an OPERATION returns to the implementation, and the processors do
differ (inf - inf is a negative NaN on x86 and a positive one on the GPU), so the definition promises NaN bits only where
nothing is computed: the copy.  same() compares accordingly: where the model holds a NaN the other side must hold a NaN,
everything else bit for bit; the tests of the copy use util.assert_bitwise.
"""
import numpy as np

from oracle.plan_model import EINVAL, ESTATE, EUNSUPPORTED, PlanModel
from util import assert_bitwise, bits

CLIP = 1
MAX = 8


def combine(f, dst, src, coef=None, c0=None, clip=False):
    """-> (f_new, sum)"""
    f = np.asarray(f)
    dt = f.dtype
    assert f.ndim == 4
    n, nxp6, nzm, T = f.shape
    nx = nxp6 - 6
    src = [int(t) for t in src]
    nsrc = len(src)
    assert 0 <= nsrc <= MAX and 0 <= dst < T and all(0 <= t < T for t in src) and (nsrc > 0 or c0 is not None)
    assert coef is None or (np.asarray(coef).dtype == dt and np.asarray(coef).shape == (n, nzm, nsrc)), (coef.dtype, coef.shape)
    assert c0 is None or (np.asarray(c0).dtype == dt and np.asarray(c0).shape == (n, nzm)), (c0.dtype, c0.shape)
    zero = dt.type(0)
    x = [np.array(f[:, 3:nx + 3, :, t]) for t in src]                # columns 1 .. nx of the OLD field
    with np.errstate(invalid="ignore", over="ignore"):
        if nsrc:
            v = np.asarray(coef)[:, None, :, 0] * x[0] if coef is not None else x[0]
            for j in range(1, nsrc):
                p = np.asarray(coef)[:, None, :, j] * x[j] if coef is not None else x[j]
                v = v + p
            if c0 is not None:
                v = v + np.asarray(c0)[:, None, :]
        else:
            v = np.broadcast_to(np.asarray(c0)[:, None, :], (n, nx, nzm))
        if clip:
            v = np.where(v > 0, v, zero)
    v = np.array(v)
    assert v.dtype == dt and v.shape == (n, nx, nzm)
    out = np.array(f, order="F")
    out[:, 3:nx + 3, :, dst] = v
    s = np.zeros((n, nzm), dt)                                       # +0
    with np.errstate(invalid="ignore"):
        for i in range(nx):
            s = s + v[:, i]
    assert s.dtype == dt
    return np.asfortranarray(out), np.asfortranarray(s)


def combine_loops(f, dst, src, coef=None, c0=None, clip=False):
    """the definition as scalar loops, one rounded operation per statement"""
    f = np.asarray(f)
    R = f.dtype.type
    n, nxp6, nzm, T = f.shape
    nx = nxp6 - 6
    out, sm = np.array(f, order="F"), np.zeros((n, nzm), f.dtype, order="F")
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(n):
            for k in range(nzm):
                s = R(0)
                for i in range(3, nx + 3):
                    if len(src):
                        v = f[b, i, k, src[0]]
                        if coef is not None:
                            v = R(coef[b, k, 0] * v)
                        for j in range(1, len(src)):
                            p = f[b, i, k, src[j]]
                            if coef is not None:
                                p = R(coef[b, k, j] * p)
                            v = R(v + p)
                        if c0 is not None:
                            v = R(v + c0[b, k])
                    else:
                        v = c0[b, k]
                    if clip:
                        v = v if v > 0 else R(0)
                    out[b, i, k, dst] = v
                    s = R(s + v)
                sm[b, k] = s
    return out, sm


def same(got, want, what=""):
    """got is want bit for bit, but that a NaN of want is met by any NaN (see the head of this file)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaNs in other places ({int(np.isnan(got).sum())} vs {int(nan.sum())})"
    assert_bitwise(np.where(nan, got.dtype.type(0), got), np.where(nan, got.dtype.type(0), want), what)


# ---- inputs.  coef: signed, of magnitude 0.25 .. 2, another value per instance, level and source, so that sums cancel in
# part and the clip bites on about half of the cells of a signed field; c0: signed, in (-1, 1).
def make_coef(n, nz, nsrc, dtype=np.float64, seed=0):
    """coef (n, nzm, nsrc), Fortran order"""
    rng = np.random.default_rng([seed, n, nz, nsrc, 21])
    c = rng.uniform(0.25, 2.0, (n, nz - 1, nsrc)) * rng.choice([-1.0, 1.0], (n, nz - 1, nsrc))
    return np.asfortranarray(c.astype(dtype))


def make_c0(n, nz, dtype=np.float64, seed=0):
    """c0 (n, nzm) in (-1, 1), Fortran order"""
    rng = np.random.default_rng([seed, n, nz, 22])
    return np.asfortranarray(rng.uniform(-1.0, 1.0, (n, nz - 1)).astype(dtype))


def call_args(n, nz, nsrc, dtype, seed, coef, c0):
    """(coef or None, c0 or None) of a call; without a source c0 is always made"""
    return (make_coef(n, nz, nsrc, dtype, seed) if coef and nsrc else None, make_c0(n, nz, dtype, seed) if c0 or not nsrc else None)


def nan_payload(dtype, k):
    """a quiet NaN with the payload k and, for odd k, the sign bit"""
    dt = np.dtype(dtype)
    if dt == np.float64:
        u = np.uint64(0x7FF8000000000000 | (k & 0xFFFF) | ((k & 1) << 63))
    else:
        u = np.uint32(0x7FC00000 | (k & 0xFFFF) | ((k & 1) << 31))
    return np.array([u]).view(dt)[0]


def plant_specials(f):
    """f (n, nx+6, nzm, T) with -0.0, +inf, -inf and NaNs (with payloads and both signs) in the interior of every tracer:
    per tracer t, level k and instance b the cell of column 1 + (b + k + t) % nx holds, by (k + 2 t) % 8: 0: -0.0, 2: +inf,
    4: a NaN with a payload, 6: -inf (only where nx > 1, else every row would end in a NaN); the others keep their value.
    -> (a copy of f, the mask of the planted cells)"""
    f = np.array(f, order="F")
    n, nxp6, nzm, T = f.shape
    nx = nxp6 - 6
    mask = np.zeros(f.shape, bool)
    for t in range(T):
        for k in range(nzm):
            for b in range(n):
                what = (k + 2 * t) % 8
                if what % 2 or (what and nx == 1 and (b + k) % 3):
                    continue
                i = 3 + (b + k + t) % nx
                f[b, i, k, t] = (-0.0, None, np.inf, None, nan_payload(f.dtype, 7 * k + b + t + 1), None, -np.inf)[what]
                mask[b, i, k, t] = True
    return np.asfortranarray(f), mask


def make_plan_inputs(oracle, shape, T=4, dtype=np.float64, seed=100, zeros=True):
    """the seven arrays of a plan, as convert_model.make_plan_inputs makes them: f signed, in [-0.5, 0.5), with -0.0 planted
    where a run keeps them (zeros)"""
    import convert_model
    return convert_model.make_plan_inputs(oracle, shape, T, dtype, seed, zeros=zeros)


class PlanModelCombine(PlanModel):
    """oracle.plan_model.PlanModel with section 3z: the call is an export of the block, the operator and an import of tracer
    dst.  The block rule: only instances [sl0, sl0 + n) of tracer dst change.  The error order: the block (n, sl0), the
    handle, the range, dst, nsrc, a missing src, the sources, a missing c0 without a source, the mode, the precision of a
    host form, the state.  The interior-only rule: halo columns are neither read nor written.  The periodic rule: no wrap is
    part of the call and the plan clears its halo mark of dst ALONE; every read-back and run of the model wraps again, as
    the plan does with cleared marks, and a source's halos are what they were -- wrapping them again changes nothing of a
    field whose interior the call has not touched.  The windowed rule (that of 3t): the plan reads and writes owned levels
    only and clears the seam mark of dst alone; the model holds the tall column, which is what the owners hold."""
    multi = False

    def combine(self, dst, src, coef=None, c0=None, mode=0, sl0=0, n=None, eb=None):
        """-> sum (n, nzm), or the code.  src: a sequence of tracers, or None (the null pointer)"""
        ncrms, nx, nz, T = self.dims
        n = ncrms - sl0 if n is None else n
        if n < 1 or sl0 < 0:
            return EINVAL
        if self.multi:
            return EUNSUPPORTED
        if sl0 + n > ncrms:
            return EINVAL
        if not 0 <= dst < T:
            return EINVAL
        nsrc = src if isinstance(src, int) else 0 if src is None else len(src)      # (an int: nsrc with a null src)
        if not 0 <= nsrc <= MAX:
            return EINVAL
        if nsrc > 0 and (src is None or isinstance(src, int)):
            return EINVAL
        if any(not 0 <= t < T for t in (src or ())):
            return EINVAL
        if nsrc == 0 and c0 is None:
            return EINVAL
        if mode & ~CLIP:
            return EINVAL
        if eb is not None and eb != np.dtype(self.dtype).itemsize:
            return ESTATE
        if not self.uploaded:
            return ESTATE
        new, s = combine(self.a["f"][sl0:sl0 + n], dst, src or (), coef, c0, bool(mode & CLIP))
        self.a["f"][sl0:sl0 + n] = new
        with np.errstate(invalid="ignore"):
            self._note()
        return s
