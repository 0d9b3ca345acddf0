"""The model of the running column integrals (include/mpdata_hip.h 3aa) in plain numpy, the inputs its tests share, and the
plan model with the new call.

column_scan(f, src, dst, wgt, mode): the arrays of ONE block in the reference layout -- f (n, nx+6, nzm, T), wgt (n, nzm) ->
(f_new, total (n, nx)).  An explicit loop over k, every statement one elementwise operation on arrays of f's dtype, hence
one rounding per element, in the definition's association: the product first, then the add; no cumsum.  Every f is read
from the OLD field, also where dst == src.  Only the interior columns 1 .. nx (array index 3 .. nx+2) of tracer dst of f_new
differ from f; halo columns are not read.  column_scan_loops is the same as a scalar triple loop, statement by statement.
scan_carried is the form a windowed plan computes: a range of levels with the running s handed in and out.
"""
import numpy as np

from oracle.plan_model import EINVAL, ESTATE, EUNSUPPORTED, PlanModel

DOWN = 1
EXCLUSIVE = 2
MODES = (0, DOWN, EXCLUSIVE, DOWN | EXCLUSIVE)


def scan_carried(x, w, s, levels, exclusive):
    """x (n, nx, nzm), w (n, nzm), the running sum s (n, nx) -> (o of the given levels, in their order: a dict level -> (n, nx);
    the new s).  levels: the order of the walk."""
    o = {}
    for k in levels:
        p = w[:, None, k] * x[:, :, k]                      # rounded to the dtype
        assert p.dtype == x.dtype
        t = s + p
        o[k] = s if exclusive else t
        s = t
    return o, s


def weights(rho, adz):
    """wgt NULL: rho * adz, one rounded multiply, as 3k forms it"""
    rho, adz = np.asarray(rho), np.asarray(adz)
    w = rho * adz
    assert w.dtype == rho.dtype == adz.dtype
    return np.asfortranarray(w)


def column_scan(f, src, dst, wgt, mode=0):
    """-> (f_new, total)"""
    f, wgt = np.asarray(f), np.asarray(wgt)
    dt = f.dtype
    assert f.ndim == 4 and mode in MODES
    n, nxp6, nzm, T = f.shape
    nx = nxp6 - 6
    assert 0 <= src < T and 0 <= dst < T and wgt.dtype == dt and wgt.shape == (n, nzm), (wgt.dtype, wgt.shape)
    x = np.array(f[:, 3:nx + 3, :, src])                    # columns 1 .. nx of the OLD field
    levels = range(nzm - 1, -1, -1) if mode & DOWN else range(nzm)
    o, s = scan_carried(x, wgt, np.zeros((n, nx), dt), levels, bool(mode & EXCLUSIVE))   # s = +0.0
    out = np.array(f, order="F")
    for k in levels:
        out[:, 3:nx + 3, k, dst] = o[k]
    assert s.dtype == dt and out.dtype == dt
    return np.asfortranarray(out), np.asfortranarray(s)


def column_scan_loops(f, src, dst, wgt, mode=0):
    """the definition as scalar loops, one rounded operation per statement"""
    f = np.asarray(f)
    R = f.dtype.type
    n, nxp6, nzm, T = f.shape
    nx = nxp6 - 6
    out, tot = np.array(f, order="F"), np.zeros((n, nx), f.dtype, order="F")
    for b in range(n):
        for i in range(nx):
            s = R(0)
            for k in (range(nzm - 1, -1, -1) if mode & DOWN else range(nzm)):
                p = R(wgt[b, k] * f[b, i + 3, k, src])
                if mode & EXCLUSIVE:
                    out[b, i + 3, k, dst] = s
                    s = R(s + p)
                else:
                    s = R(s + p)
                    out[b, i + 3, k, dst] = s
            tot[b, i] = s
    return out, tot


# ---- inputs.  wgt: signed, of magnitude 0.25 .. 1, another value per instance and level, so that the running sum of a
# signed f in [-0.5, 0.5) cancels in part and stays below nzm / 2 in magnitude: chains of calls and runs stay finite.
def make_wgt(n, nz, dtype=np.float64, seed=0):
    """wgt (n, nzm), Fortran order"""
    rng = np.random.default_rng([seed, n, nz, 31])
    w = rng.uniform(0.25, 1.0, (n, nz - 1)) * rng.choice([-1.0, 1.0], (n, nz - 1))
    return np.asfortranarray(w.astype(dtype))


def make_plan_inputs(oracle, shape, T=3, dtype=np.float64, seed=100):
    """the seven arrays of a plan, as vsolve_model.make_plan_inputs makes them: f signed, in [-0.5, 0.5); rho and adz in
    [0.5, 1)"""
    import vsolve_model
    return vsolve_model.make_plan_inputs(oracle, shape, T, dtype, seed)


class PlanModelColumnScan(PlanModel):
    """oracle.plan_model.PlanModel with section 3aa: the call is an export of the block, the scan and an import of tracer
    dst.  The block rule: only instances [sl0, sl0 + n) of tracer dst change.  The error order: the block (n, sl0), the
    handle, the range, src, dst, the mode, the precision of a host form, the state.  The interior-only rule: halo columns are
    neither read nor written.  The periodic rule: no wrap is part of the call and the plan clears its halo mark of dst ALONE;
    every read-back and run of the model wraps again, as the plan does with cleared marks, and the halos of src are what
    they were.  The windowed rule: the plan reads and writes owned levels only, carries s from window to window and clears
    the seam mark of dst alone; the model holds the tall column, which is what the owners hold.  The phantom and the
    partner of a split pair have no face here: no export reads the phantom, and the partner is another instance, which
    the block rule keeps."""
    multi = False

    def column_scan(self, src, dst, wgt=None, mode=0, sl0=0, n=None, eb=None):
        """-> total (n, nx), or the code.  wgt None: rho * adz of the model"""
        ncrms, nx, nz, T = self.dims
        n = ncrms - sl0 if n is None else n
        if n < 1 or sl0 < 0:
            return EINVAL
        if self.multi:
            return EUNSUPPORTED
        if sl0 + n > ncrms:
            return EINVAL
        if not 0 <= src < T or not 0 <= dst < T:
            return EINVAL
        if mode & ~(DOWN | EXCLUSIVE):
            return EINVAL
        if eb is not None and eb != np.dtype(self.dtype).itemsize:
            return ESTATE
        if not self.uploaded:
            return ESTATE
        b = slice(sl0, sl0 + n)
        w = weights(self.a["rho"][b], self.a["adz"][b]) if wgt is None else wgt
        new, tot = column_scan(self.a["f"][b], src, dst, w, mode)
        self.a["f"][b] = new
        self._note()
        return tot
