"""GPU tests of the implicit vertical diffusion of a resident plan with a per-cell diffusivity (include/mpdata_hip.h 3s):
mpdata_plan_vdiffuse_device, the host forms, the array forms, their Python face Plan.vdiffuse / vdiffuse_host / vdiffuse,
and the Fortran program tests/fortran/vdiffuse_calls.F90.

Every comparison is bit for bit (util.assert_bitwise) against the numpy model of tests/vdiffuse_model.py: DV.vdiffuse on a
reference-layout truth, or the plan model with the new call (DV.PlanModelVdiffuse: an EXACT plan's f and flux are
bit-identical to it), or, for FAST plans, the plan's own whole export before the call.  The whole export of f AND flux is
compared.  tkh, cz, sb, st lie inside larger buffers with 4 KiB of NaN on both sides, which must come back unchanged, and
in EVERY call of this file the device copies of tkh's columns 0 and nx+1 and of cz(:, nzm) are NaN as well: a read of
either poisons the result.  tkh is zero in a third of the cells and in a column now and then, cz uniform in [0, 2), rho and
adz in [0.5, 1): the off-diagonals reach 16.  f is the oracle's raw field moved by one half, so signed.  u and w have no
export: that they keep their bits shows in the run behind the calls, which is compared with the model's.

G = 16 is the group of the kernel: the adjacent 8-byte elements of the instance axis a workgroup owns (4 at 237 levels).
CB = 4 is the column batch of the kernel as built at 27 levels ((2560 / (16 * 27)) - 1: a cell takes two LDS elements, so
the geometry is that of half the 40 KiB), so nx = 11 is three batches of 4, 4 and 3; at 71 levels and above a batch is 1
column.  Shapes (ncrms, nx, nz): 37 instances are two full groups and a partial one, 5 less than one, 1 a single lane;
nx = 1, 3 and 11; 1 and 3 tracers; nz = 2 (one level: the array forms only, a plan has 3 or more), 3 (one interface), 12,
28 (two slots per tile), 34 (one slot), 65, 66 (two slices), 72, 130, 238 (the tallest plain plan: the smallest group).
fp32: pairs (even, 37 pairs), the phantom (odd with the switch), the reference layout (odd without it)."""
import numpy as np
import pytest

import fortran_records as FR
import plan_harness as H
import vdiffuse_model as DV
import vsolve_model as VM
from oracle import plan_model as PM
from plan_harness import _defaults, nan_banded, upload
from util import assert_bitwise, to_dev, to_host

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
G = 16

# name -> (shape, tracers, dtype, switches)
KINDS = {
    "f64-nz3": ((5, 11, 3), 3, F64, {}),
    "f64-nz28": ((5, 1, 28), 1, F64, {}), "f64-nz28-3groups": ((2 * G + 5, 11, 28), 3, F64, {}),
    "f64-nz28-n1": ((1, 3, 28), 1, F64, {}),
    "f64-nz34": ((5, 11, 34), 1, F64, {}), "f64-nz65": ((5, 1, 65), 1, F64, {}), "f64-nz66": ((5, 11, 66), 1, F64, {}),
    "f64-nz72": ((5, 3, 72), 3, F64, {}), "f64-nz130": ((5, 1, 130), 1, F64, {}), "f64-nz238": ((5, 3, 238), 1, F64, {}),
    "f32-nz28-even": ((6, 11, 28), 3, F32, {}), "f32-nz28-3groups": ((4 * G + 10, 1, 28), 1, F32, {}),
    "f32-nz72-even": ((6, 3, 72), 1, F32, {}),
    "f32-nz28-odd": ((2 * G + 5, 11, 28), 3, F32, dict(odd=True)), "f32-nz72-odd": ((5, 1, 72), 1, F32, dict(odd=True)),
    "f32-nz3-odd": ((5, 3, 3), 1, F32, dict(odd=True)),
    "f64-nz12-ref": ((5, 3, 12), 3, F64, dict(ref=True)),
    "f32-nz28-odd-ref": ((5, 3, 28), 1, F32, {}),      # (an odd fp32 plan without the switch keeps the reference layout)
}
REF = ("f64-nz12-ref", "f32-nz28-odd-ref")
# one kind of each family runs the FAST variant too; one of each a PERIODIC plan
FAST = ("f64-nz28-3groups", "f64-nz72", "f32-nz28-odd", "f64-nz12-ref")
PERIODIC = ("f64-nz34", "f32-nz72-odd", "f64-nz12-ref", "f32-nz28-even")
# which of sb, st a kind's first call carries (the later calls rotate through all four)
FLUXES = ((True, True), (True, False), (False, True), (False, False))
SEED = 100


_INPUTS = {}


def inputs(oracle, name):
    """the seven arrays of KINDS[name]: computed once and shared; no test writes them"""
    if name not in _INPUTS:
        shape, T, dt, _ = KINDS[name]
        _INPUTS[name] = DV.make_plan_inputs(oracle, shape, T, dt, SEED)
    return _INPUTS[name]


def new_plan(M, name, variant=None):
    return H.new_plan(M, KINDS[name], name, name in REF, False, variant)


def model_of(oracle, name):
    shape, T, dt, _ = KINDS[name]
    m = DV.PlanModelVdiffuse(oracle, *shape, T, dt)
    assert m.upload({k: np.array(v, order="F") for k, v in inputs(oracle, name).items()}) is None
    return m


def whole(M, p, name, what=("f", "flux")):
    return H.whole(M, p, KINDS[name], what)


def same_as_model(M, p, name, m, what):
    H.same_as_model(M, p, KINDS[name], name, m, what)


def coeffs_of(name, k, n=None, **kw):
    """{tkh, cz, sb, st} of a block, other values per k; the fluxes present as FLUXES[k % 4] says"""
    shape, T, dt, _ = KINDS[name]
    c = DV.make_coeffs(shape[0] if n is None else n, shape[1], shape[2], dt, 500 + k, **kw)
    sb, st = FLUXES[k % 4]
    if not sb:
        c["sb"] = None
    if not st:
        c["st"] = None
    return c


def poisoned(c):
    """the device copy of a call's arrays: NaN where the call must not read"""
    tkh, cz = np.array(c["tkh"], order="F"), np.array(c["cz"], order="F")
    tkh[:, 0] = np.nan
    tkh[:, -1] = np.nan
    cz[:, -1] = np.nan
    return dict(c, tkh=tkh, cz=cz)


def device_arrays(M, c, n, nx, nz):
    """-> ([(raw, pristine copy, view) or None per array], the four views)"""
    sh = M.vdiffuse_shapes(n, nx, nz)
    bufs = []
    for k in ("tkh", "cz", "sb", "st"):
        if c[k] is None:
            bufs.append(None)
            continue
        raw, view = nan_banded(c[k], sh[k])
        bufs.append((raw, raw.clone(), view))
    return bufs, [None if b is None else b[2] for b in bufs]


def unchanged(bufs):
    import torch
    for b, k in zip(bufs, ("tkh", "cz", "sb", "st")):
        assert b is None or torch.equal(b[0].view(torch.uint8), b[1].view(torch.uint8)), f"{k} changed"


def vdiffuse(M, p, name, c, sl0=0, n=None, first=0, ntr=None, call=None):
    """Plan.vdiffuse of the host arrays c between NaN bands, poisoned where the call must not read; all are checked
    unchanged.  call: another callable with Plan.vdiffuse's arguments (a shard plan's)."""
    import torch
    shape, T, dt, _ = KINDS[name]
    n = shape[0] - sl0 if n is None else n
    ntr = T - first if ntr is None else ntr
    assert c["tkh"].shape == (n, shape[1] + 2, shape[2] - 1) and c["tkh"].dtype == dt
    bufs, views = device_arrays(M, poisoned(c), n, shape[1], shape[2])
    torch.cuda.synchronize()      # (the plan may run on a stream that does not wait for the one that filled the buffers)
    (call or p.vdiffuse)(*views, sl0, n, first, ntr)
    p.sync()
    torch.cuda.synchronize()
    unchanged(bufs)


def mcall(m, c, **kw):
    return m.vdiffuse(c["tkh"], c["cz"], c["sb"], c["st"], **kw)


def model_f(F, inp, c, sl0=0, n=None):
    n = F.shape[0] - sl0 if n is None else n
    return DV.vdiffuse(F, inp["rho"][sl0:sl0 + n], inp["adz"][sl0:sl0 + n], c["tkh"], c["cz"], c["sb"], c["st"])


# ---- 1. every kind of plan: upload -> vdiffuse -> compare -> run -> compare -> vdiffuse twice -> compare (-> run -> compare)
@pytest.mark.parametrize("name", list(KINDS))
def test_every_plan_kind(mpdata, oracle, name):
    M = mpdata
    shape, T, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    inp = inputs(oracle, name)
    F0 = inp["f"].reshape((ncrms, nx + 6, nz - 1, T), order="F")
    p = new_plan(M, name)
    upload(p, inp)
    m = model_of(oracle, name)
    # (a) upload -> vdiffuse -> the model on the uploaded f
    c0 = coeffs_of(name, list(KINDS).index(name))
    assert (F0 < 0).any() and (F0 > 0).any()
    vdiffuse(M, p, name, c0)
    want_f = model_f(F0, inp, c0)
    assert_bitwise(want_f[:, :3], F0[:, :3], "the halos stay")
    assert_bitwise(want_f[:, nx + 3:], F0[:, nx + 3:], "the halos stay")
    assert not np.array_equal(want_f, F0)
    assert mcall(m, c0) is None
    e = whole(M, p, name)
    assert_bitwise(e["f"], want_f, f"{name} (a): f")
    assert_bitwise(e["flux"], inp["flux"].reshape(e["flux"].shape, order="F"), f"{name} (a): flux")
    same_as_model(M, p, name, m, "(a) the plan model")
    # (b) a run on the kept velocities = export -> model -> import -> run: the phantom is consistent
    p.run()
    assert m.run() is None
    same_as_model(M, p, name, m, "(b) vdiffuse, run")
    # (c) behind the run, twice in a row, with other fluxes present
    for k in (1, 2):
        c = coeffs_of(name, k)
        vdiffuse(M, p, name, c)
        assert mcall(m, c) is None
    same_as_model(M, p, name, m, "(c) run, vdiffuse, vdiffuse")
    p.run()
    assert m.run() is None
    same_as_model(M, p, name, m, "(c) run, vdiffuse, vdiffuse, run")
    if name in PERIODIC:
        # (d) PERIODIC: run, vdiffuse while the halos are stale; the export hands out wrapped halos of the NEW field
        p.set_boundary(M.BOUNDARY_PERIODIC)
        assert m.set_boundary(PM.PERIODIC) is None
        p.run()
        assert m.run() is None
        c = coeffs_of(name, 5)
        vdiffuse(M, p, name, c)
        assert mcall(m, c) is None
        same_as_model(M, p, name, m, "(d) periodic: run, vdiffuse")
        # ... on halos the export just wrapped: they are copies of the OLD field now, the next export wraps again
        c = coeffs_of(name, 6)
        vdiffuse(M, p, name, c)
        assert mcall(m, c) is None
        e = whole(M, p, name, ("f",))["f"]
        assert_bitwise(e, PM.wrap(np.array(e, order="F")), f"{name} (d): the halos are wrapped copies of the new interior")
        same_as_model(M, p, name, m, "(d) periodic: vdiffuse on wrapped halos")
        c = coeffs_of(name, 7)
        vdiffuse(M, p, name, c)
        assert mcall(m, c) is None
        p.run()
        assert m.run() is None
        same_as_model(M, p, name, m, "(d) periodic: vdiffuse, run")
        # ... and back to GIVEN behind a call: the plan holds what an export just before the switch would have returned
        c = coeffs_of(name, 8)
        vdiffuse(M, p, name, c)
        assert mcall(m, c) is None
        p.set_boundary(M.BOUNDARY_GIVEN)
        assert m.set_boundary(PM.GIVEN) is None
        same_as_model(M, p, name, m, "(d) periodic: vdiffuse, set_boundary(GIVEN)")
    p.close()
    if name in FAST:
        # FAST: the same bits as EXACT on the uploaded f; after a run against the plan's own export changed by the model
        p = new_plan(M, name, variant=M.VARIANT_FAST)
        upload(p, inp)
        vdiffuse(M, p, name, c0)
        assert_bitwise(whole(M, p, name, ("f",))["f"], want_f, f"{name} FAST upload, vdiffuse")
        p.run()
        E = whole(M, p, name, ("f",))["f"]
        c1 = coeffs_of(name, 1)
        vdiffuse(M, p, name, c1)
        assert_bitwise(whole(M, p, name, ("f",))["f"], model_f(E, inp, c1), f"{name} FAST run, vdiffuse")
        p.close()


# ---- 2. blocks and tracer sub-ranges: what lies outside keeps every bit
BLOCKS = {
    # two per tile, five instances: inside one group, one instance, the last one
    "f64-nz28": [(1, 3), (2, 1), (4, 1), (0, 5)],
    # three groups: a block that straddles a group boundary, odd sl0 across two boundaries, the last instance alone, a group
    "f64-nz28-3groups": [(G - 1, 3), (3, 2 * G), (2 * G + 4, 1), (G, G)],
    "f64-nz72": [(1, 1), (1, 2)],
    "f64-nz238": [(1, 1), (3, 2), (0, 5)],
    # fp32 pairs: odd sl0 and odd n (split pairs at both ends), one half, a whole pair
    "f32-nz28-even": [(1, 3), (5, 1), (2, 2)],
    # 37 pairs: across a group boundary (2G instances per group), splitting pairs
    "f32-nz28-3groups": [(2 * G - 1, 3), (1, 4 * G + 4), (4 * G + 9, 1)],
    # fp32 pairs, odd plan of 37 (instance 36 shares its pair with the phantom): blocks that hold and miss instance 36
    "f32-nz28-odd": [(1, 2), (36, 1), (35, 2), (0, 36), (33, 3), (0, 37)],
    "f32-nz72-odd": [(4, 1), (1, 1), (0, 2), (3, 2)],
    "f32-nz28-odd-ref": [(1, 3), (4, 1)],
    "f64-nz12-ref": [(1, 3), (4, 1)],
}


@pytest.mark.parametrize("name", list(BLOCKS))
def test_blocks_leave_the_rest_alone(mpdata, oracle, name):
    M = mpdata
    shape, T, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    inp = inputs(oracle, name)
    p = new_plan(M, name)
    upload(p, inp)
    m = model_of(oracle, name)
    for k, (sl0, n) in enumerate(BLOCKS[name]):
        first, ntr = ((k % T), 1) if T > 1 else (0, 1)
        if T > 1 and k == len(BLOCKS[name]) - 1:
            first, ntr = 0, T
        if T > 2 and k == 1:
            first, ntr = 1, 2
        before = whole(M, p, name)
        c = coeffs_of(name, 10 + k, n)
        vdiffuse(M, p, name, c, sl0, n, first, ntr)
        assert mcall(m, c, sl0=sl0, n=n, first=first, ntr=ntr) is None
        after = whole(M, p, name)
        out = np.ones(ncrms, bool)
        out[sl0:sl0 + n] = False
        tout = np.ones(T, bool)
        tout[first:first + ntr] = False
        assert_bitwise(after["f"][out], before["f"][out], f"{name} block {sl0, n}: instances outside")
        assert_bitwise(after["f"][..., tout], before["f"][..., tout], f"{name} block {sl0, n}: tracers outside")
        assert_bitwise(after["flux"], before["flux"], f"{name} block {sl0, n}: flux")
        want = model_f(before["f"][sl0:sl0 + n, ..., first:first + ntr], inp, c, sl0, n)
        assert_bitwise(after["f"][sl0:sl0 + n, ..., first:first + ntr], want, f"{name} block {sl0, n}: inside")
        assert not np.array_equal(want, before["f"][sl0:sl0 + n, ..., first:first + ntr])
        # a run of every instance (the phantom of an odd plan rides with instance ncrms - 1; u, w, rho, rhow, adz enter
        # it) matches the model
        p.run()
        assert m.run() is None
        same_as_model(M, p, name, m, f"block {sl0, n}, run")
    p.close()


# ---- 3. x-uniform tkh: Plan.vsolve on a twin plan with lo = -a, di, up = -c gives the same bits, on the GPU
@pytest.mark.parametrize("name", ["f64-nz28-3groups", "f32-nz28-odd", "f64-nz12-ref"])
def test_x_uniform_equals_vsolve_on_a_twin(mpdata, oracle, name):
    M = mpdata
    shape, T, dt, sw = KINDS[name]
    inp = inputs(oracle, name)
    c = coeffs_of(name, 3, x_uniform=True)                 # (FLUXES[3]: no sb, no st)
    assert c["sb"] is None and c["st"] is None and (c["tkh"] == c["tkh"][:, 1:2]).all() and (c["tkh"][:, 1] != c["tkh"][:1, 1]).any()
    _, a, cc, di = DV.coefficients(inp["rho"], inp["adz"], c["tkh"], c["cz"])
    lo, di, up = (np.asfortranarray(x[:, 0]) for x in (-a, di, -cc))
    p, q = new_plan(M, name), new_plan(M, name)
    upload(p, inp)
    upload(q, inp)
    vdiffuse(M, p, name, c)
    q.vsolve(to_dev(lo), to_dev(di), to_dev(up), 0, shape[0], 0, T)
    q.sync()
    got, twin = whole(M, p, name), whole(M, q, name)
    assert not np.array_equal(got["f"], inp["f"].reshape(got["f"].shape, order="F"))
    for k in got:
        assert_bitwise(got[k], twin[k], f"{name}: vdiffuse with an x-uniform tkh against vsolve: {k}")
    p.close()
    q.close()


# ---- 4. the host forms equal the device form (both equal the model bit for bit)
@pytest.mark.parametrize("name", ["f64-nz28-3groups", "f32-nz28-odd", "f64-nz12-ref", "f64-nz72"])
def test_host_form(mpdata, oracle, name):
    M = mpdata
    shape, T, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    p = new_plan(M, name)
    upload(p, inputs(oracle, name))
    m = model_of(oracle, name)
    for k, (sl0, n) in enumerate(((0, ncrms), (1, 1), (ncrms - 1, 1), (0, 2))):
        c = coeffs_of(name, 20 + k, n)
        h = poisoned(c)
        keep = {kk: None if v is None else np.array(v, order="F") for kk, v in h.items()}
        p.vdiffuse_host(h["tkh"], h["cz"], h["sb"], h["st"], sl0, n)
        for kk in h:
            assert h[kk] is None or h[kk].tobytes("F") == keep[kk].tobytes("F"), f"{name} host {sl0, n}: {kk}"
        assert mcall(m, c, sl0=sl0, n=n) is None
        same_as_model(M, p, name, m, f"host form {sl0, n}")
        p.run()
        assert m.run() is None
        same_as_model(M, p, name, m, f"host form {sl0, n}, run")
    with pytest.raises(M.MpdataError):
        p.vdiffuse_host(c["tkh"][:, :-1], c["cz"], sl0=0, n=2)       # a wrong shape
    p.close()


# 257 and 600 instances: more than one block of 256 threads and a partly filled last one; (2, 65538, 3): 65538 columns, the
# second trip over gridDim.y; (2, 1, 3) with 32769 tracers: the tracers inside the thread.  f is random, so instance b
# differs from b - 256 and column i from i - 65535.  Each with a block inside the arrays; f lies between NaN bands that
# must come back unchanged.  (5, 1, 2): one level, which no plan can have (mpdata_plan_create needs nz >= 3).
ARRAYS = {"nz2": ((5, 1, 2), 1, (1, 3)), "n257": ((257, 3, 6), 2, (1, 256)), "n600": ((600, 2, 5), 1, (300, 299)),
          "rows65538": ((2, 1, 3), 32769, (1, 1)), "cols65538": ((2, 65538, 3), 1, (1, 1))}


@pytest.mark.parametrize("case", list(ARRAYS))
@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
def test_array_forms(mpdata, dt, case):
    import torch
    M = mpdata
    (ncrms, nx, nz), T, (b0, bn) = ARRAYS[case]
    rng = np.random.default_rng([77, ncrms, T])
    f = np.asfortranarray(rng.uniform(-1.0, 1.0, (ncrms, nx + 6, nz - 1, T)).astype(dt))
    rho, adz = (np.asfortranarray(rng.uniform(0.5, 1.0, (ncrms, nz - 1)).astype(dt)) for _ in range(2))
    drho, dadz = to_dev(rho), to_dev(adz)
    for sl0, n in ((0, ncrms), (b0, bn)):
        c = DV.make_coeffs(n, nx, nz, dt, 600 + sl0)
        full = np.array(f, order="F")
        full[sl0:sl0 + n] = DV.vdiffuse(f[sl0:sl0 + n], rho[sl0:sl0 + n], adz[sl0:sl0 + n], c["tkh"], c["cz"], c["sb"], c["st"])
        if n > 256:
            assert not np.array_equal(full[sl0 + 256:sl0 + n], full[sl0:sl0 + n - 256])
        if nx > 65535:
            assert not np.array_equal(full[:, 3 + 65535:nx + 3], full[:, 3:nx + 3 - 65535])
        fraw, fd = nan_banded(f, (T, nz - 1, nx + 6, ncrms))
        pad = (fraw.numel() - fd.numel()) // 2
        bufs, views = device_arrays(M, poisoned(c), n, nx, nz)
        torch.cuda.synchronize()
        M.vdiffuse(fd, drho, dadz, *views, sl0, n)
        torch.cuda.synchronize()
        assert torch.isnan(fraw[:pad]).all() and torch.isnan(fraw[-pad:]).all(), "a guard band of f changed"
        unchanged(bufs)
        assert_bitwise(to_host(fd), full, f"array form {case} block {sl0, n}: f")
    if T == 1 or case == "n257":
        # one tracer without the tracer axis, no boundary fluxes
        f1 = to_dev(np.asfortranarray(f[..., 0]))
        c = DV.make_coeffs(ncrms, nx, nz, dt, 650, fluxes=False)
        M.vdiffuse(f1, drho, dadz, to_dev(c["tkh"]), to_dev(c["cz"]))
        torch.cuda.synchronize()
        assert_bitwise(to_host(f1), DV.vdiffuse(f[..., 0], rho, adz, c["tkh"], c["cz"]), f"array form {case}, one tracer: f")


# ---- 5. every error code, in the stated order; the plan's state before and after
def test_errors_change_nothing(mpdata, oracle):
    M = mpdata
    name = "f64-nz72"
    shape, T, dt, _ = KINDS[name]
    ncrms, nx, nz = shape
    inp = inputs(oracle, name)
    c = coeffs_of(name, 0)
    dev = [to_dev(c[k]) for k in ("tkh", "cz", "sb", "st")]

    def code(fn, *a, **kw):
        with pytest.raises(M.MpdataError) as e:
            fn(*a, **kw)
        return e.value.code

    p = new_plan(M, name)
    assert code(p.vdiffuse, *dev) == M.ESTATE                                      # never filled
    upload(p, inp)
    before = whole(M, p, name)
    L = M.lib()
    ptr = [a.data_ptr() for a in dev]
    raw = lambda sl0, n, first, ntr, a=ptr: L.mpdata_plan_vdiffuse_device(p._p, sl0, n, a[0], a[1], a[2], a[3], first, ntr)
    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, ncrms + 1), (ncrms, 1), (3, 3)):
        assert raw(sl0, n, 0, 1) == M.EINVAL, (sl0, n)
    for first, ntr in ((0, 0), (-1, 1), (2, 2), (3, 1), (0, 4)):
        assert raw(0, ncrms, first, ntr) == M.EINVAL, (first, ntr)
    for i, nm in enumerate(("tkh", "cz")):
        a = list(ptr)
        a[i] = None
        assert raw(0, ncrms, 0, 1, a) == M.EINVAL and b"null " + nm.encode() in L.mpdata_last_error()
        assert raw(0, 0, 0, 1, a) == M.EINVAL and b"n = 0" in L.mpdata_last_error()                # the range first
        assert raw(0, ncrms, 0, 4, a) == M.EINVAL and b"tracer range" in L.mpdata_last_error()     # then the tracers
    # a host form of the other precision; its NULL comes first
    h32 = [np.asfortranarray(c[k].astype(F32)) for k in ("tkh", "cz", "sb", "st")]
    assert L.mpdata_plan_vdiffuse_f32(p._p, 0, ncrms, *(a.ctypes.data for a in h32)) == M.ESTATE
    assert L.mpdata_plan_vdiffuse_f32(p._p, 0, ncrms, h32[0].ctypes.data, None, None, None) == M.EINVAL
    assert b"null cz" in L.mpdata_last_error()
    after = whole(M, p, name)
    for k in before:
        assert_bitwise(after[k], before[k], f"after the refused calls: {k}")
    p.vdiffuse(*dev)                                                               # ... and the plan still works
    p.sync()
    assert not np.array_equal(whole(M, p, name, ("f",))["f"], before["f"])
    p.close()


# ---- 6. a windowed plan is refused, behind the NULLs and in front of the state, and keeps every bit
def test_windowed_plan_is_refused(mpdata, oracle):
    M = mpdata
    kind = ((3, 2, 239), 1, F64, dict(tall=True))
    shape, T, dt, _ = kind
    inp = DV.make_plan_inputs(oracle, shape, T, dt, SEED)
    c = DV.make_coeffs(shape[0], shape[1], shape[2], dt, 900)
    dev = [to_dev(c[k]) for k in ("tkh", "cz", "sb", "st")]
    p = H.new_plan(M, kind, "f64-nz239-tall", False, True)
    L = M.lib()
    with pytest.raises(M.MpdataError) as e:                                        # (never filled: the window comes first)
        p.vdiffuse(*dev)
    assert e.value.code == M.EUNSUPPORTED and b"windowed" in L.mpdata_last_error()
    upload(p, inp)
    before = H.whole(M, p, kind)
    with pytest.raises(M.MpdataError) as e:
        p.vdiffuse(*dev)
    assert e.value.code == M.EUNSUPPORTED
    with pytest.raises(M.MpdataError) as e:
        p.vdiffuse_host(c["tkh"], c["cz"], c["sb"], c["st"])
    assert e.value.code == M.EUNSUPPORTED
    assert L.mpdata_plan_vdiffuse_device(p._p, 0, shape[0], None, dev[1].data_ptr(), None, None, 0, 1) == M.EINVAL   # the NULL first
    after = H.whole(M, p, kind)
    for k in before:
        assert_bitwise(after[k], before[k], f"after the refused calls: {k}")
    p.close()


# ---- 7. a multi-GPU handle is refused; the single-device plans of its shards take the call
def test_multi_gpu_handle_and_shard_plan(mpdata, oracle, monkeypatch):
    M = mpdata
    monkeypatch.delenv("MPDATA_MULTI_XFER", raising=False)
    name = "f64-nz72"
    shape, T, dt, _ = KINDS[name]
    inp = inputs(oracle, name)
    p = M.Plan(*shape, T, dtype=dt, devices=[0, 0])
    upload(p, inp)
    m = model_of(oracle, name)
    c = coeffs_of(name, 40)
    with pytest.raises(M.MpdataError) as e:
        p.vdiffuse(*(None if c[k] is None else to_dev(c[k]) for k in ("tkh", "cz", "sb", "st")))
    assert e.value.code == M.EUNSUPPORTED and b"mpdata_plan_shard_plan" in M.lib().mpdata_last_error()
    with pytest.raises(M.MpdataError) as e:
        p.vdiffuse_host(c["tkh"], c["cz"], c["sb"], c["st"])
    assert e.value.code == M.EUNSUPPORTED
    same_as_model(M, p, name, m, "after the refused handle calls")
    for g, (_, s0, nloc) in enumerate(p.shards()):
        q = p.shard_plan(g)
        cg = coeffs_of(name, 41 + g, nloc)
        vdiffuse(M, q, name, cg, 0, nloc, 0, T, call=q.vdiffuse)
        assert mcall(m, cg, sl0=s0, n=nloc) is None
        q.close()
    same_as_model(M, p, name, m, "after the shard plans' calls")
    p.run()
    assert m.run() is None
    same_as_model(M, p, name, m, "after the shard plans' calls and a run")
    p.close()


# ---- 8. the Fortran program: every record of its dump against the model
FORTRAN = {
    "f64": (F64, "vdiffuse_calls", (7, 5, 10), 3, (2, 3), (1, 2)), "f32-odd-ref": (F32, "vdiffuse_calls_sp", (7, 3, 12), 2, (6, 1), (1, 1)),
}


@pytest.mark.parametrize("case", list(FORTRAN))
def test_fortran_program_matches_the_model(oracle, tmp_path, case):
    dt, exe, shape, T, (sl0, n), (t1, tn) = FORTRAN[case]
    ncrms, nx, nz = shape
    inp = DV.make_plan_inputs(oracle, shape, T, dt, SEED + 3)
    arrs = {k: (inp[k].reshape(inp[k].shape + (1,), order="F") if T == 1 and k in ("f", "flux") else inp[k]) for k in PM.NAMES}
    ca, cb = DV.make_coeffs(n, nx, nz, dt, 700), DV.make_coeffs(ncrms, nx, nz, dt, 701, fluxes=False)
    records = [("params", np.array([ncrms, nx, nz, T, sl0, n, t1, tn], np.int64))]
    records += [(k, arrs[k]) for k in PM.NAMES]
    records += [(k + "_a", ca[k]) for k in ("tkh", "cz", "sb", "st")] + [(k + "_b", cb[k]) for k in ("tkh", "cz")]
    # the replay on the model
    m = DV.PlanModelVdiffuse(oracle, ncrms, nx, nz, T, dt)
    want = FR.want_import(m, inp)
    rc = lambda what, code=None: want.append(FR.rc(what, code))
    rc("vd_block", mcall(m, ca, sl0=sl0, n=n)); rc("sync")
    e = m.export_device()
    rc("export"); rc("sync")
    want += [("f_a", e["f"]), ("flux_a", e["flux"])]
    rc("vd_range", mcall(m, cb, first=t1, ntr=tn)); rc("sync")
    want += FR.want_close(m)
    FR.compare_dump(FR.run_program(exe, records, tmp_path), want, case)
