"""The model of the fused column step (include/mpdata_hip.h 3q) in plain numpy, the inputs its tests share, and the plan
model with the new call.

column_step(f, rho, adz, s, c, mode, cb, cc, wp, lo, di, up): the arrays of ONE block in the reference layout -- f (n,
nx+6, nzm[, T]) -- -> (f_new, psfc (n, nx[, T]) or None).  It COMPOSES the models of the single sections in the fixed order
of 3q -- cell_add_model.cell_add, subside_model.subside, sediment_model.sediment, vsolve_model.vsolve --, a stage present
exactly when its arrays are given, so every operation has the rounding and the association those models state.  psfc is
the sediment model's, hence of the field that enters that stage.  After the subside stage the halo columns are restored
from the input: 3m alone also updates them, the fused call does not touch them.  No horizontal sum is returned.
"""
import numpy as np

import cell_add_model as CM
import sediment_model as SM
import subside_model as UM
import vsolve_model as VM
from oracle.plan_model import EINVAL, ESTATE, EUNSUPPORTED, PlanModel
from util import bits

ADD, CLIP = CM.ADD, CM.CLIP
STAGES = ("source", "subside", "sediment", "vsolve")
# the 15 non-empty subsets of the stages, as tuples of names in the fixed order
SUBSETS = [tuple(st for b, st in enumerate(STAGES) if mask >> b & 1) for mask in range(1, 16)]


def column_step(f, rho=None, adz=None, s=None, c=1.0, mode=ADD, cb=None, cc=None, wp=None, lo=None, di=None, up=None):
    f = np.asarray(f)
    nx = f.shape[1] - 6
    assert (cb is None) == (cc is None) and (lo is None) == (di is None) == (up is None)
    assert s is not None or cb is not None or wp is not None or lo is not None
    g = np.array(f, order="F")
    psfc = None
    if s is not None:
        g, _ = CM.cell_add(g, s, c, mode)
    if cb is not None:
        g, _ = UM.subside(g, cb, cc)
        g = np.array(g, order="F")
        g[:, :3], g[:, nx + 3:] = f[:, :3], f[:, nx + 3:]          # the halo columns are not touched
    if wp is not None:
        g, psfc, _ = SM.sediment(g, rho, adz, wp)
    if lo is not None:
        g = VM.vsolve(g, lo, di, up)
    assert g.dtype == f.dtype and g.shape == f.shape
    return np.asfortranarray(g), psfc


# ---- inputs: the make_* helpers of the single sections, one seed per call
def make_args(n, nx, nz, T=None, dtype=np.float64, seed=0, stages=STAGES):
    """the keyword arguments of column_step / PlanModelColumnStep.column_step for the given stages (without c and mode): s
    and wp (n, nx, nzm[, T]), cb, cc, lo, di, up (n, nzm)"""
    kw = {}
    if "source" in stages:
        kw["s"] = CM.make_s(n, nx, nz, T, dtype, seed)
    if "subside" in stages:
        kw["cb"], kw["cc"] = UM.make_coeffs(n, nz, dtype, seed + 1)
    if "sediment" in stages:
        kw["wp"] = SM.make_wp(n, nx, nz, T, dtype, seed + 2)
    if "vsolve" in stages:
        kw["lo"], kw["di"], kw["up"] = VM.make_coeffs(n, nz, dtype, seed + 3)
    return kw


def make_plan_inputs(oracle, shape, T=1, dtype=np.float64, seed=100):
    """the seven arrays of a plan, as subside_model.make_plan_inputs makes them: f signed, in [-0.5, 0.5), no -0.0; rho and
    adz in [0.5, 1); f and flux carry a tracer axis only for T > 1"""
    return UM.make_plan_inputs(oracle, shape, T, dtype, seed)


class PlanModelColumnStep(PlanModel):
    """oracle.plan_model.PlanModel with section 3q.  The block rule: only instances [sl0, sl0 + n) and tracers [first,
    first + ntr) change.  The error order: the block, the handle, the range, the tracers, the NULLs (no stage; one of cb,
    cc; one or two of lo, di, up; psfc without wp), the mode while s is given, the windowed plan, the precision of a host
    form, the state.  The interior-only rule: halo columns are neither read nor written.  The periodic rule: no wrap is part
    of the call and the plan clears its halo marks; every read-back and run of the model wraps again, as the plan does with
    cleared marks.  windowed: the plan is one of level windows, which the call refuses."""
    multi = False
    windowed = False

    def column_step(self, s=None, c=1.0, mode=ADD, cb=None, cc=None, wp=None, psfc=False, lo=None, di=None, up=None, sl0=0, n=None,
                    first=0, ntr=None, eb=None):
        """-> psfc with a tracer axis (None without wp), or the code; psfc: the caller passes an array for it"""
        ncrms, nx, nz, T = self.dims
        n = ncrms - sl0 if n is None else n
        ntr = T - first if ntr is None else ntr
        if n < 1 or sl0 < 0:
            return EINVAL
        if self.multi:
            return EUNSUPPORTED
        if sl0 + n > ncrms or not self._tracers_ok(first, ntr):
            return EINVAL
        nv = sum(x is not None for x in (lo, di, up))
        if s is None and cb is None and cc is None and wp is None and nv == 0 and not psfc:
            return EINVAL
        if (cb is None) != (cc is None) or nv in (1, 2) or (psfc and wp is None):
            return EINVAL
        if s is not None and mode not in (ADD, CLIP):
            return EINVAL
        if self.windowed:
            return EUNSUPPORTED
        if eb is not None and eb != np.dtype(self.dtype).itemsize:
            return ESTATE
        if not self.uploaded:
            return ESTATE

        def axis(a):
            a = np.asarray(a)
            return a.reshape(a.shape + (1,)) if a.ndim == 3 else a

        blk = self.a["f"][sl0:sl0 + n, ..., first:first + ntr]
        new, ps = column_step(blk, self.a["rho"][sl0:sl0 + n], self.a["adz"][sl0:sl0 + n], None if s is None else axis(s), c, mode,
                              cb, cc, None if wp is None else axis(wp), lo, di, up)
        self.a["f"][sl0:sl0 + n, ..., first:first + ntr] = new
        self._note()
        return ps
