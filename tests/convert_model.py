"""The model of the first-order conversion between two tracers (include/mpdata_hip.h 3t) in plain numpy, the inputs its
tests share, and the plan model with the new call.

convert(f, src, dst, r, q0, y, limit): the arrays of ONE block in the reference layout -- f (n, nx+6, nzm, T), r (n, nzm),
q0, y (n, nzm) or None -- -> (f_new, dsum (n, nzm)).  Every statement below is one elementwise operation on arrays of f's
dtype, hence one rounding per element, in the definition's association; the comparisons are np.where on a plain `>`, so NaN
and -0 fall to the +0 branch as in the definition; dsum is an explicit loop over i = 1 .. nx from +0.  Levels with r == 0
(either sign) are copied, not computed, and their dsum is +0.  Only the interior columns 1 .. nx (array index 3 .. nx+2) of
tracers src and dst of f_new differ from f; halo columns and other tracers are not read.  convert_loops is the same as a
scalar triple loop, statement by statement.
"""
import numpy as np

from oracle.plan_model import EINVAL, ESTATE, EUNSUPPORTED, PlanModel
from util import bits

LIMIT = 1


def convert(f, src, dst, r, q0=None, y=None, limit=False, parts=False):
    """-> (f_new, dsum); parts: -> (f_new, dsum, d, e_raw, capped) with d (n, nx, nzm) the amount moved, e_raw the argument
    of the threshold select and capped the cells where the LIMIT cap replaced d (what the tests' branch counts need)"""
    f = np.asarray(f)
    dt = f.dtype
    assert f.ndim == 4 and src != dst
    n, nxp6, nzm, T = f.shape
    nx = nxp6 - 6
    zero = dt.type(0)
    for x in (r, q0, y):
        assert x is None or (np.asarray(x).dtype == dt and np.asarray(x).shape == (n, nzm)), (x.dtype, x.shape, (n, nzm))
    a = np.array(f[:, 3:nx + 3, :, src])                    # columns 1 .. nx
    c = np.array(f[:, 3:nx + 3, :, dst])
    rr = np.asarray(r)[:, None, :]
    e_raw = a - np.asarray(q0)[:, None, :] if q0 is not None else a
    e = np.where(e_raw > 0, e_raw, zero)
    d = rr * e
    capped = np.zeros(d.shape, bool)
    if limit:
        m = np.where(a > 0, a, zero)
        capped = d > m
        d = np.where(capped, m, d)
    na = a - d
    g = np.asarray(y)[:, None, :] * d if y is not None else d
    nc = c + g
    for x in (e, d, na, g, nc):
        assert x.dtype == dt
    on = np.broadcast_to(rr != 0, a.shape)                  # r == 0: the level keeps every bit
    out = np.array(f, order="F")
    out[:, 3:nx + 3, :, src] = np.where(on, na, a)
    out[:, 3:nx + 3, :, dst] = np.where(on, nc, c)
    s = np.zeros((n, nzm), dt)                              # +0
    for i in range(nx):
        s = np.where(on[:, i], s + d[:, i], s)
    assert s.dtype == dt
    if parts:
        return np.asfortranarray(out), np.asfortranarray(s), d, e_raw, capped
    return np.asfortranarray(out), np.asfortranarray(s)


def convert_loops(f, src, dst, r, q0=None, y=None, limit=False):
    """the definition as scalar loops, one rounded operation per statement"""
    f = np.asarray(f)
    R = f.dtype.type
    n, nxp6, nzm, T = f.shape
    nx = nxp6 - 6
    out, dsum = np.array(f, order="F"), np.zeros((n, nzm), f.dtype, order="F")
    for b in range(n):
        for k in range(nzm):
            if r[b, k] == 0:
                continue
            s = R(0)
            for i in range(3, nx + 3):
                a, c = f[b, i, k, src], f[b, i, k, dst]
                e = R(a - q0[b, k]) if q0 is not None else a
                e = e if e > 0 else R(0)
                d = R(r[b, k] * e)
                if limit:
                    m = a if a > 0 else R(0)
                    d = m if d > m else d
                out[b, i, k, src] = R(a - d)
                g = R(y[b, k] * d) if y is not None else d
                out[b, i, k, dst] = R(c + g)
                s = R(s + d)
            dsum[b, k] = s
    return out, dsum


def branch_shares(f, src, dst, r, q0=None, y=None, limit=False, sl0=0, n=None):
    """what the GPU tests assert on the model before every call, of the block [sl0, sl0 + n) of f (n, nx+6, nzm, T):
    (share of the touched cells of src the call changes bitwise, share of the cells of the converting levels that take
    the e <= 0 branch, share of the converted cells -- e > 0 on a converting level -- where the LIMIT cap is active)"""
    f = np.asarray(f)
    n = f.shape[0] - sl0 if n is None else n
    nx = f.shape[1] - 6
    blk = np.asfortranarray(f[sl0:sl0 + n])
    new, _, d, e_raw, capped = convert(blk, src, dst, r, q0, y, limit, parts=True)
    changed = float(np.mean(bits(new[:, 3:nx + 3, :, src]) != bits(blk[:, 3:nx + 3, :, src])))
    on = np.broadcast_to((np.asarray(r) != 0)[:, None, :], d.shape)
    off = float(np.mean(~(e_raw[on] > 0))) if on.any() else 0.0
    conv = on & (e_raw > 0)
    cap = float(np.mean(capped[conv])) if conv.any() else 0.0
    return changed, off, cap


# ---- inputs.  r: zero on the lower half of the levels, uniform in (0, 2] above, so that with LIMIT the cap bites where
# r > 1; every instance and level has its own value.  q0: a value of f's own interior per (instance, level) -- the column of
# rank (nx - 1) // 2, the lower median --, so at least a third of the cells take the e <= 0 branch, at least one converts
# at any nx >= 2, and one cell per row has a == q0 exactly.  y: uniform in [0.5, 1.5).
def make_r(n, nz, dtype=np.float64, seed=0):
    """r (n, nzm), Fortran order"""
    rng = np.random.default_rng([seed, n, nz, 11])
    nzm = nz - 1
    r = 2.0 - rng.uniform(0.0, 2.0, (n, nzm))               # (0, 2]
    r[:, :nzm // 2] = 0.0
    r = r.astype(dtype)
    r[:, nzm // 2:][r[:, nzm // 2:] == 0] = 1               # (a value that rounded to zero in fp32)
    return np.asfortranarray(r)


def make_q0(fsrc):
    """q0 (n, nzm) from tracer src of a block, fsrc (n, nx+6, nzm): the interior value of rank (nx - 1) // 2 of every row"""
    nx = fsrc.shape[1] - 6
    return np.asfortranarray(np.sort(fsrc[:, 3:nx + 3], axis=1)[:, (nx - 1) // 2])


def make_y(n, nz, dtype=np.float64, seed=0):
    """y (n, nzm) in [0.5, 1.5), Fortran order"""
    rng = np.random.default_rng([seed, n, nz, 12])
    return np.asfortranarray(rng.uniform(0.5, 1.5, (n, nz - 1)).astype(dtype))


def plant_negative_zeros(oracle, inp, mask):
    """inp with f = -0.0 on the cells of mask (f's shape, with the tracer axis) -> (inp, the mask that stayed).  The plan
    kernels and the oracle do not agree on the sign of the zero a RUN returns for a cell that held -0.0 and met no flux
    (every face an outflow face: the run's clamp at zero sees -0.0; nothing of 3t is involved), so a cell whose first run
    from these inputs returns a -0.0 gets its value back.  The tests assert on the model that no run of theirs returns a
    -0.0."""
    f0 = np.array(inp["f"], order="F")
    mask = np.array(mask)
    n, nxp6, nzm, T = f0.shape
    for _ in range(4):
        f = np.array(f0, order="F")
        f[mask] = -0.0
        m = PlanModel(oracle, n, nxp6 - 6, nzm + 1, T, f0.dtype)
        arrs = {k: np.array(v, order="F") for k, v in inp.items()}
        arrs["f"] = f
        assert m.upload(arrs) is None and m.run() is None
        bad = mask & (m.a["f"] == 0) & np.signbit(m.a["f"])
        if not bad.any():
            break
        mask &= ~bad
    else:
        raise AssertionError("the planted -0.0 do not settle")
    out = dict(inp)
    out["f"] = np.asfortranarray(f)
    return out, mask


def make_plan_inputs(oracle, shape, T=3, dtype=np.float64, seed=100, raw=False, zeros=True):
    """the seven arrays of a plan, as subside_model.make_plan_inputs makes them: f signed, in [-0.5, 0.5) (raw: the oracle's
    raw field, in [0, 1)); zeros: some -0.0 are planted in the interior of every tracer (column 2, every third level; see
    plant_negative_zeros)"""
    import subside_model
    inp = dict(subside_model.make_plan_inputs(oracle, shape, T, dtype, seed))
    f = np.array(inp["f"], order="F")
    if raw:
        f = f + np.dtype(dtype).type(0.5)
    inp["f"] = np.asfortranarray(f)
    if not zeros:
        return inp
    mask = np.zeros(f.shape, bool)
    mask[:, 4, ::3] = True
    inp, mask = plant_negative_zeros(oracle, inp, mask)
    assert mask.sum() * 2 > f.shape[0] * ((f.shape[2] + 2) // 3) * T        # most of them stay
    return inp


class PlanModelConvert(PlanModel):
    """oracle.plan_model.PlanModel with section 3t: the call is an export of the two tracers of the block, the operator and
    an import.  The block rule: only instances [sl0, sl0 + n) and tracers src and dst change.  The error order: the block
    (n, sl0), the handle, the range, the pair (outside, then equal), the NULL r, the mode, the precision of a host form, the
    state.  The interior-only rule: halo columns are neither read nor written.  The periodic rule: no wrap is part of the
    call and the plan clears its halo marks of both tracers; every read-back and run of the model wraps again, as the plan
    does with cleared marks.  The windowed rule (that of 3r): the plan reads and writes owned levels only and clears the
    seam marks of both tracers; the model holds the tall column, which is what the owners hold."""
    multi = False

    def convert(self, src, dst, r, q0=None, y=None, mode=0, sl0=0, n=None, eb=None):
        """-> dsum (n, nzm), or the code"""
        ncrms, nx, nz, T = self.dims
        n = ncrms - sl0 if n is None else n
        if n < 1 or sl0 < 0:
            return EINVAL
        if self.multi:
            return EUNSUPPORTED
        if sl0 + n > ncrms:
            return EINVAL
        if not (0 <= src < T and 0 <= dst < T) or src == dst:
            return EINVAL
        if r is None or mode & ~LIMIT:
            return EINVAL
        if eb is not None and eb != np.dtype(self.dtype).itemsize:
            return ESTATE
        if not self.uploaded:
            return ESTATE
        new, dsum = convert(self.a["f"][sl0:sl0 + n], src, dst, r, q0, y, bool(mode & LIMIT))
        self.a["f"][sl0:sl0 + n] = new
        self._note()
        return dsum
