"""The model of the outflow Courant number (include/mpdata_hip.h 3h) in plain numpy, and the inputs its tests share.

courant(u, w, rho, adz): reference-layout arrays u (ncrms, nx+5, nzm), w (ncrms, nx+4, nz), rho, adz (ncrms, nzm).  Per
instance sl, interior column i = 1 .. nx (array index i + 1 of u and w) and level k = 1 .. nzm

    a = max(0, u(i+1,k)) - min(0, u(i,k))
    b = max(0, wk1) - min(0, w(i,k))         wk1 = w(i,k+1) for k < nzm, +0 for k = nzm (w(:, nz) is never read)
    c = (a + b * iadz) * irho                iadz = 1 / adz, irho = 1 / rho

every operation elementwise in the arrays' dtype and as a statement of its own -- an explicit loop over i, never a fused
expression --, the sign of c cleared; clev = max over i, cinst = max over k.  WRONG holds the named wrong variants the
input guard of tests/test_courant_cpu.py checks against.
"""
import numpy as np

import level_stats_model as LM

bits = LM.bits


def _courant(u, w, rho, adz, variant=None):
    u, w, rho, adz = (np.asarray(x) for x in (u, w, rho, adz))
    dt = u.dtype
    assert w.dtype == dt and rho.dtype == dt and adz.dtype == dt
    ncrms, nxp5, nzm = u.shape
    nx = nxp5 - 5
    assert nx >= 1 and w.shape == (ncrms, nx + 4, nzm + 1) and rho.shape == adz.shape == (ncrms, nzm)
    zero = np.zeros((ncrms, nzm), dt)                          # +0.0
    one = np.ones((), dt)
    iadz = one / adz
    irho = one / rho
    clev = np.zeros((ncrms, nzm), dt)
    cols = range(1, nx + 1)
    if variant == "columns_0_to_nx-1":
        cols = range(0, nx)
    elif variant == "columns_2_to_nx+1":
        cols = range(2, nx + 2)
    for i in cols:
        u0 = u[:, i + 1]                                       # u(i, :)
        u1 = u[:, i + 2]                                       # u(i+1, :)
        w0 = w[:, i + 1, :nzm]                                 # w(i, 1..nzm)
        w1 = np.concatenate([w[:, i + 1, 1:nzm], zero[:, :1]], axis=1)   # w(i, k+1), +0 at k = nzm
        if variant == "u_swapped":
            u0, u1 = u1, u0
        elif variant == "w_below":
            w1 = np.concatenate([zero[:, :1], w[:, i + 1, :nzm - 1]], axis=1)   # w(i, k-1)
        elif variant == "w_top_read":
            w1 = w[:, i + 1, 1:nzm + 1]                        # the caller's w(:, nz) at the top level
        if variant == "abs_faces":
            a = np.maximum(np.abs(u1), np.abs(u0))
            b = np.maximum(np.abs(w1), np.abs(w0))
        else:
            a = np.maximum(zero, u1)
            a = a - np.minimum(zero, u0)
            b = np.maximum(zero, w1)
            b = b - np.minimum(zero, w0)
        if variant == "sum_then_scale":
            c = a + b
            c = c * iadz
            c = c * irho
        elif variant == "divides":
            c = b / adz
            c = a + c
            c = c / rho
        else:
            c = b * iadz
            c = a + c
            c = c * irho
        c = np.abs(c)                                          # the sign is cleared: a zero is +0.0
        assert c.dtype == dt
        clev = np.maximum(clev, c)
    cinst = np.zeros((ncrms,), dt)
    for k in range(nzm):
        cinst = np.maximum(cinst, clev[:, k])
    return np.asfortranarray(clev), cinst


def courant(u, w, rho, adz):
    """-> (clev (ncrms, nzm) Fortran order, cinst (ncrms,))"""
    return _courant(u, w, rho, adz)


# the wrong variants of the input guard: 1. inflow instead of outflow, 2. w(k-1) for w(k+1), 3. the caller's w(:, nz) at
# the top level, 4. |u|, |w| face maxima instead of the signed parts, 5. (a + b) * iadz * irho, 6. (a + b / adz) / rho,
# 7. columns 0 .. nx-1 or 2 .. nx+1 instead of 1 .. nx
WRONG = ("u_swapped", "w_below", "w_top_read", "abs_faces", "sum_then_scale", "divides", "columns_0_to_nx-1", "columns_2_to_nx+1")


def wrong(name, u, w, rho, adz):
    assert name in WRONG
    return _courant(u, w, rho, adz, name)


# ---- inputs: level_stats_model.make (oracle.DIST_RAW_SIGNED: u, w in [-0.5, 0.5), rho, adz in [0, 1) with every element
# drawn on its own, so a column of rho, adz has as many distinct values as it has levels) with w(:, :, nz) set to values
# that are not zero (and up to 2 in size, so that reading them shows in a max), and rho, adz moved away from zero by +0.5.
def make(oracle, name):
    """the seven arrays of level_stats_model.INPUTS[name] (f: all its tracers), seed from SEEDS"""
    shape, T, dt, _ = LM.INPUTS[name]
    inp = LM.make(oracle, shape, T, dt, SEEDS[name])
    w = np.array(inp["w"], order="F")
    top = oracle.make_inputs(*shape, seed=SEEDS[name] + 1000, dist=oracle.DIST_RAW_SIGNED, dtype=dt)["w"][:, :, 0]
    w[:, :, -1] = np.where(top == 0, dt(0.25), top) * dt(4)
    inp["w"] = w
    for k in ("rho", "adz"):
        inp[k] = np.asfortranarray(inp[k] + dt(0.5))
        assert inp[k].dtype == dt and np.all(inp[k] >= 0.5)
    assert np.all(w[:, :, -1] != 0)
    return inp


def other(oracle, name, shift=50):
    """a second set of velocities of the same shape (imports, run_uw)"""
    shape, T, dt, _ = LM.INPUTS[name]
    o = oracle.make_inputs(*shape, seed=SEEDS[name] + shift, dist=oracle.DIST_RAW_SIGNED, dtype=dt)
    return o["u"], o["w"]


# every entry of level_stats_model.INPUTS: the seeds at which each wrong variant differs from the model in at least one
# element of clev (tests/test_courant_cpu.py asserts the condition; nothing here is measured).
SEEDS = {k: v[3] for k, v in LM.INPUTS.items()}
