"""GPU tests of the sedimentation of a resident plan (include/mpdata_hip.h 3n): mpdata_plan_sediment_device, the host
forms, the array forms, their Python face Plan.sediment / sediment_host / sediment, and the Fortran program
tests/fortran/sediment_calls.F90.

Every comparison is bit for bit (util.assert_bitwise) against the numpy model of tests/sediment_model.py: SM.sediment on a
reference-layout truth, or the plan model with the new call (SM.PlanModelSediment: an EXACT plan's f and flux are
bit-identical to it), or, for FAST plans, the plan's own whole export before the call.  wp lies inside a larger buffer with
4 KiB of NaN on both sides, so a read outside the block's array poisons the result; psfc and pflux are filled with NaN and
lie between two patterned bands of 4 KiB, which must come back unchanged, and so must wp.  wp is uniform in [-0.05, 0.2),
another value per cell and tracer; f is the oracle's raw field moved by one half, so signed.  u and w have no export: that
they keep their bits shows in the run behind every call, which is compared with the model's.

G = 16 is the group of the kernel: the adjacent 8-byte elements of the instance axis a workgroup owns.  Shapes (ncrms, nx,
nz): the smallest at which a path of the kernel differs.  (5, 3, 8): padding slots of an 8-instance tile, a group of 32;
(5, 11, 28): two column batches, the second short; (3, 3, 64): 63 elements, four rounds; (2G+5, 3, 28): three groups, the
last short; (3, 2, 65), (3, 9, 72): element 63 | 64 across two waves, batches of 3 columns; (2, 2, 140): three slices, an
idle wave; (2, 2, 238): four slices, a group of 4.  fp32: pairs (even), 2G+3 pairs, the phantom (odd with the switch), the
reference layout (odd without it).  Windowed plans (nz > 238 with set_tall_columns): 239 and 300 levels, G+2 instances
(two groups), fp32 with 15 pseudo-instances (an inner phantom); 250 levels without the switch is a reference-layout plan."""
import numpy as np
import pytest

import fortran_records as FR
import plan_harness as H
import sediment_model as SM
from oracle import plan_model as PM
from plan_harness import BAND, _defaults, nan_banded, nan_out, upload
from util import assert_bitwise, to_dev, to_host

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
G = 16

# name -> (shape, tracers, dtype, switches)
KINDS = {
    "f64-nz8": ((5, 3, 8), 2, F64, {}), "f64-nz28-nx11": ((5, 11, 28), 2, F64, {}), "f64-nz64": ((3, 3, 64), 1, F64, {}),
    "f64-nz28-3groups": ((2 * G + 5, 3, 28), 1, F64, {}),
    "f64-nz65": ((3, 2, 65), 1, F64, {}), "f64-nz72": ((3, 9, 72), 2, F64, {}), "f64-nz140": ((2, 2, 140), 1, F64, {}),
    "f64-nz238": ((2, 2, 238), 1, F64, {}),
    "f32-nz28-even": ((6, 3, 28), 2, F32, {}), "f32-nz28-3groups": ((4 * G + 6, 3, 28), 1, F32, {}),
    "f32-nz72-even": ((4, 2, 72), 1, F32, {}),
    "f32-nz28-odd": ((7, 3, 28), 2, F32, dict(odd=True)), "f32-nz72-odd": ((3, 2, 72), 1, F32, dict(odd=True)),
    "f64-nz12-ref": ((5, 3, 12), 2, F64, dict(ref=True)), "f32-nz12-ref": ((6, 3, 12), 2, F32, dict(ref=True)),
    "f32-nz12-odd-ref": ((7, 3, 12), 1, F32, {}),      # (an odd fp32 plan without the switch keeps the reference layout)
    "f64-nz250-ref": ((2, 3, 250), 1, F64, {}),        # (above 238 levels without the switch: the reference layout)
    "f64-nz239-tall": ((2, 3, 239), 2, F64, dict(tall=True)), "f64-nz300-tall": ((3, 2, 300), 1, F64, dict(tall=True)),
    "f64-nz239-tall-2groups": ((G + 2, 2, 239), 1, F64, dict(tall=True)),
    "f32-nz239-tall-odd": ((3, 2, 239), 2, F32, dict(tall=True, odd=True)),
}
REF = ("f32-nz12-odd-ref", "f64-nz12-ref", "f32-nz12-ref", "f64-nz250-ref")
# one kind of each family runs the FAST variant too; three kinds run a PERIODIC plan
FAST = ("f64-nz28-nx11", "f64-nz72", "f32-nz28-odd", "f64-nz12-ref", "f64-nz239-tall")
PERIODIC = ("f64-nz28-nx11", "f32-nz72-odd", "f64-nz12-ref", "f32-nz239-tall-odd")
SEED = 100


_INPUTS = {}


def inputs(oracle, name):
    """the seven arrays of KINDS[name]: computed once and shared; no test writes them"""
    if name not in _INPUTS:
        shape, T, dt, _ = KINDS[name]
        _INPUTS[name] = SM.make_plan_inputs(oracle, shape, T, dt, SEED)
    return _INPUTS[name]


def new_plan(M, name, variant=None):
    return H.new_plan(M, KINDS[name], name, name in REF, bool(KINDS[name][3].get("tall")), variant)


def model_of(oracle, name):
    shape, T, dt, _ = KINDS[name]
    m = SM.PlanModelSediment(oracle, *shape, T, dt)
    assert m.upload({k: np.array(v, order="F") for k, v in inputs(oracle, name).items()}) is None
    return m


def whole(M, p, name, what=("f", "flux")):
    return H.whole(M, p, KINDS[name], what)


def same_as_model(M, p, name, m, what):
    H.same_as_model(M, p, KINDS[name], name, m, what)


def wp_of(name, k, n=None, ntr=None):
    """wp (n, nx, nzm, ntr) of a block, another field per k"""
    shape, T, dt, _ = KINDS[name]
    return SM.make_wp(shape[0] if n is None else n, shape[1], shape[2], T if ntr is None else ntr, dt, 500 + k)


def sediment(M, p, name, wp, sl0=0, n=None, first=0, ntr=None, outs=("psfc", "pflux"), lead=None, call=None):
    """Plan.sediment of a host wp (n, nx, nzm, ntr) -> (psfc (n, nx, ntr) or None, pflux (n, nzm, ntr) or None); wp and the
    bands are checked.  call: another callable with Plan.sediment's arguments (a shard plan's, the array form's)."""
    import torch
    shape, T, dt, _ = KINDS[name]
    nx, nz = shape[1], shape[2]
    n = shape[0] - sl0 if n is None else n
    ntr = T - first if ntr is None else ntr
    assert wp.shape == (n, nx, nz - 1, ntr) and wp.dtype == dt
    lead = (ntr != 1) if lead is None else lead
    sh = M.sediment_shapes(n, nx, nz, ntr if lead else None)
    wraw, wview = nan_banded(wp, sh["wp"])
    worig = wraw.clone()
    bufs = {k: nan_out(sh[k], dt) for k in outs}
    torch.cuda.synchronize()      # (the plan may run on a stream that does not wait for the one that filled the buffers)
    (call or p.sediment)(wview, bufs["psfc"][2] if "psfc" in bufs else None, bufs["pflux"][2] if "pflux" in bufs else None, sl0, n,
                         first, ntr)
    p.sync()
    torch.cuda.synchronize()
    assert torch.equal(wraw.view(torch.uint8), worig.view(torch.uint8)), "wp changed"
    out = []
    for k, w in (("psfc", nx), ("pflux", nz - 1)):
        if k not in bufs:
            out.append(None)
            continue
        raw, pristine, view = bufs[k]
        assert torch.equal(raw[:BAND], pristine[:BAND]) and torch.equal(raw[-BAND:], pristine[-BAND:]), f"{k}: a band byte changed"
        out.append(to_host(view).reshape((n, w, ntr), order="F"))
    return tuple(out)


def check_outs(got, want, what):
    for k, g, w in zip(("psfc", "pflux"), got, want):
        if g is not None:
            assert_bitwise(g, w, f"{what}: {k}")


# ---- 1. every kind of plan: whole plan, every state, the three subsets of the optional arrays
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
    # (a) upload -> sediment with both outputs -> the model on the uploaded f
    w0 = wp_of(name, 0)
    assert (w0 < 0).any() and (w0 > 0).any() and (F0 < 0).any() and (F0 > 0).any()
    got = sediment(M, p, name, w0)
    want_f, want_s, want_p = SM.sediment(F0, inp["rho"], inp["adz"], w0)
    assert_bitwise(want_f[:, :3], F0[:, :3], "the halos stay")
    assert_bitwise(want_f[:, nx + 3:], F0[:, nx + 3:], "the halos stay")
    assert not np.array_equal(want_f, F0)
    check_outs(got, (want_s, want_p), f"{name} (a)")
    check_outs(got, m.sediment(w0), f"{name} (a) the plan model")
    e = whole(M, p, name)
    assert_bitwise(e["f"], want_f, f"{name} (a): f")
    assert_bitwise(e["flux"], inp["flux"].reshape(e["flux"].shape, order="F"), f"{name} (a): flux")
    # (b) a run on the kept velocities = export -> model -> import -> run: seams and the phantom are consistent
    p.run()
    assert m.run() is None
    same_as_model(M, p, name, m, "(b) sediment, run")
    # (c) behind the run (a windowed plan's seams are stale): psfc alone, pflux alone, neither; a run behind each
    for k, outs in enumerate((("psfc",), ("pflux",), ())):
        w = wp_of(name, 1 + k)
        got = sediment(M, p, name, w, outs=outs)
        check_outs(got, m.sediment(w), f"{name} (c) outputs {outs}")
        same_as_model(M, p, name, m, f"(c) run, sediment with {outs}")
        p.run()
        assert m.run() is None
        same_as_model(M, p, name, m, f"(c) run, sediment with {outs}, run")
    if name in PERIODIC:
        # (d) PERIODIC: run, sediment while the halos are stale; the export hands out wrapped halos of the NEW field
        p.set_boundary(M.BOUNDARY_PERIODIC)
        assert m.set_boundary(PM.PERIODIC) is None
        p.run()
        assert m.run() is None
        w = wp_of(name, 5)
        check_outs(sediment(M, p, name, w), m.sediment(w), f"{name} (d) periodic, stale halos")
        same_as_model(M, p, name, m, "(d) periodic: run, sediment")
        # ... on halos the export just wrapped: they are copies of the OLD field now, the next export wraps again
        w = wp_of(name, 6)
        check_outs(sediment(M, p, name, w), m.sediment(w), f"{name} (d) periodic, wrapped halos")
        e = whole(M, p, name, ("f",))["f"]
        assert_bitwise(e, PM.wrap(np.array(e, order="F")), f"{name} (d): the halos are wrapped copies of the new interior")
        same_as_model(M, p, name, m, "(d) periodic: sediment on wrapped halos")
        w = wp_of(name, 7)
        sediment(M, p, name, w, outs=())
        assert m.sediment(w) is not None
        p.run()
        assert m.run() is None
        same_as_model(M, p, name, m, "(d) periodic: sediment, run")
        # ... and back to GIVEN behind a call: the plan holds what an export just before the switch would have returned
        w = wp_of(name, 8)
        sediment(M, p, name, w, outs=())
        assert m.sediment(w) is not None
        p.set_boundary(M.BOUNDARY_GIVEN)
        assert m.set_boundary(PM.GIVEN) is None
        same_as_model(M, p, name, m, "(d) periodic: sediment, set_boundary(GIVEN)")
    p.close()
    if name in FAST:
        # FAST: the same bits as EXACT on the uploaded f; after a run against the plan's own export changed by the model
        p = new_plan(M, name, variant=M.VARIANT_FAST)
        upload(p, inp)
        check_outs(sediment(M, p, name, w0), (want_s, want_p), f"{name} FAST")
        assert_bitwise(whole(M, p, name, ("f",))["f"], want_f, f"{name} FAST upload, sediment")
        p.run()
        E = whole(M, p, name, ("f",))["f"]
        w1 = wp_of(name, 1)
        got = sediment(M, p, name, w1)
        want_E, s_E, p_E = SM.sediment(E, inp["rho"], inp["adz"], w1)
        check_outs(got, (s_E, p_E), f"{name} FAST run, sediment")
        assert_bitwise(whole(M, p, name, ("f",))["f"], want_E, f"{name} FAST run, sediment")
        p.close()


# ---- 2. blocks and tracer sub-ranges: what lies outside keeps every bit
BLOCKS = {
    # eight instances per tile, five instances: inside the tile, one instance, the last one
    "f64-nz8": [(1, 3), (2, 1), (4, 1), (0, 5)],
    # two per tile: mid-tile to mid-tile, the last (half-filled) tile
    "f64-nz28-nx11": [(1, 3), (4, 1), (0, 4)],
    # three groups: a block that straddles a group boundary, odd sl0 across two boundaries, the last instance alone
    "f64-nz28-3groups": [(G - 1, 3), (3, 2 * G), (2 * G + 4, 1), (G, G)],
    "f64-nz72": [(1, 1), (1, 2)],
    "f64-nz140": [(1, 1), (0, 1)],
    # fp32 pairs: a block that splits pairs at both ends
    "f32-nz28-even": [(1, 3), (5, 1), (2, 2)],
    # 2G+3 pairs: across a group boundary (2G instances per group), splitting pairs
    "f32-nz28-3groups": [(2 * G - 1, 3), (1, 4 * G + 4), (4 * G + 5, 1)],
    # fp32 pairs, odd plan of 7 (instance 6 shares its pair with the phantom): blocks that hold and miss instance 6
    "f32-nz28-odd": [(1, 2), (6, 1), (5, 2), (0, 6), (3, 3), (0, 7)],
    "f32-nz72-odd": [(2, 1), (1, 1), (0, 2)],
    "f32-nz12-odd-ref": [(1, 3), (6, 1)],
    "f64-nz12-ref": [(1, 3), (4, 1)],
    # windowed plans: each behind an import (the first) and behind a run (the others: stale seams), a block and the whole
    "f64-nz239-tall": [(1, 1), (0, 1), (0, 2)],
    "f64-nz239-tall-2groups": [(G - 1, 3), (G + 1, 1), (1, G)],
    "f32-nz239-tall-odd": [(1, 1), (2, 1), (0, 2), (0, 3)],
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
        before = whole(M, p, name)
        w = wp_of(name, 10 + k, n, ntr)
        got = sediment(M, p, name, w, sl0, n, first, ntr, lead=bool(k % 2) or ntr > 1)
        check_outs(got, m.sediment(w, sl0=sl0, n=n, first=first, ntr=ntr), f"{name} block {sl0, n} tracers {first, ntr}")
        after = whole(M, p, name)
        out = np.ones(ncrms, bool)
        out[sl0:sl0 + n] = False
        tout = np.ones(T, bool)
        tout[first:first + ntr] = False
        assert_bitwise(after["f"][out], before["f"][out], f"{name} block {sl0, n}: instances outside")
        assert_bitwise(after["f"][..., tout], before["f"][..., tout], f"{name} block {sl0, n}: tracers outside")
        assert_bitwise(after["flux"], before["flux"], f"{name} block {sl0, n}: flux")
        want = SM.sediment(before["f"][sl0:sl0 + n, ..., first:first + ntr], inp["rho"][sl0:sl0 + n], inp["adz"][sl0:sl0 + n], w)[0]
        assert_bitwise(after["f"][sl0:sl0 + n, ..., first:first + ntr], want, f"{name} block {sl0, n}: inside")
        assert not np.array_equal(want, before["f"][sl0:sl0 + n, ..., first:first + ntr])
        # a run of every instance (the phantom of an odd plan rides with instance ncrms - 1; a windowed plan refreshes
        # the seams the call marked stale; u, w, rho, rhow, adz enter it) matches the model
        p.run()
        assert m.run() is None
        same_as_model(M, p, name, m, f"block {sl0, n}, run")
    p.close()


# ---- 3. the host form and the array forms
@pytest.mark.parametrize("name", ["f64-nz28-nx11", "f32-nz28-odd", "f64-nz12-ref", "f64-nz72", "f64-nz239-tall"])
def test_host_form(mpdata, oracle, name):
    M = mpdata
    shape, T, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    p = new_plan(M, name)
    upload(p, inputs(oracle, name))
    m = model_of(oracle, name)
    tail = (T,) if T > 1 else ()
    for k, (sl0, n, outs) in enumerate(((0, ncrms, ("psfc", "pflux")), (1, 1, ()), (ncrms - 1, 1, ("pflux",)), (0, 2, ("psfc",)))):
        w = wp_of(name, 20 + k, n)
        wh = np.asfortranarray(w.reshape((n, nx, nz - 1) + tail, order="F"))
        keep = np.array(wh, order="F")
        s = np.full((n, nx) + tail, np.nan, dt, order="F") if "psfc" in outs else None
        f = np.full((n, nz - 1) + tail, np.nan, dt, order="F") if "pflux" in outs else None
        p.sediment_host(wh, s, f, sl0, n)
        assert_bitwise(wh, keep, f"{name} host {sl0, n}: wp")
        ws, wf = m.sediment(w, sl0=sl0, n=n)
        if s is not None:
            assert_bitwise(s.reshape(ws.shape, order="F"), ws, f"{name} host {sl0, n}: psfc")
        if f is not None:
            assert_bitwise(f.reshape(wf.shape, order="F"), wf, f"{name} host {sl0, n}: pflux")
        same_as_model(M, p, name, m, f"host form {sl0, n}")
        # ... against the device form on a second plan is the same statement: both equal the model bit for bit
        p.run()
        assert m.run() is None
        same_as_model(M, p, name, m, f"host form {sl0, n}, run")
    with pytest.raises(M.MpdataError):
        p.sediment_host(wh[:, :, :-1], sl0=0, n=2)       # a wrong shape
    p.close()


# 257 and 600 instances: more than one block of 256 threads and a partly filled last one; (2, 1, 3) with 32769 tracers:
# 65538 rows, the second trip over gridDim.y.  f and wp are random, so instance b differs from b - 256 and row r from
# r - 65535.  Each with a block inside the arrays.
ARRAYS = {"n257": ((257, 3, 6), 2, (1, 256)), "n600": ((600, 2, 5), 1, (300, 299)), "rows65538": ((2, 1, 3), 32769, (1, 1))}


@pytest.mark.parametrize("case", list(ARRAYS))
@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
def test_array_forms(mpdata, dt, case):
    import torch
    M = mpdata
    (ncrms, nx, nz), T, (b0, bn) = ARRAYS[case]
    rng = np.random.default_rng([77, ncrms, T])
    f = np.asfortranarray(rng.uniform(-1.0, 1.0, (ncrms, nx + 6, nz - 1, T)).astype(dt))
    rho, adz = (np.asfortranarray(rng.uniform(0.5, 1.0, (ncrms, nz - 1)).astype(dt)) for _ in range(2))
    for sl0, n in ((0, ncrms), (b0, bn)):
        wp = SM.make_wp(n, nx, nz, T, dt, 600 + sl0)
        want, want_s, want_p = SM.sediment(f[sl0:sl0 + n], rho[sl0:sl0 + n], adz[sl0:sl0 + n], wp)
        full = np.array(f, order="F")
        full[sl0:sl0 + n] = want
        if n > 256:
            assert not np.array_equal(want[256:], want[:n - 256]) and not np.array_equal(want_p[256:], want_p[:n - 256])
        fd, rd, ad = to_dev(f), to_dev(rho), to_dev(adz)
        sh = M.sediment_shapes(n, nx, nz, T)
        wraw, wview = nan_banded(wp, sh["wp"])
        bs, bp = nan_out(sh["psfc"], dt), nan_out(sh["pflux"], dt)
        torch.cuda.synchronize()
        M.sediment(fd, rd, ad, wview, bs[2], bp[2], sl0, n)
        torch.cuda.synchronize()
        for raw, pristine, _ in (bs, bp):
            assert torch.equal(raw[:BAND], pristine[:BAND]) and torch.equal(raw[-BAND:], pristine[-BAND:])
        assert_bitwise(to_host(fd), full, f"array form {case} block {sl0, n}: f")
        assert_bitwise(to_host(bs[2]), want_s, f"array form {case} block {sl0, n}: psfc")
        assert_bitwise(to_host(bp[2]), want_p, f"array form {case} block {sl0, n}: pflux")
        assert_bitwise(to_host(rd), rho, "rho")
        assert_bitwise(to_host(ad), adz, "adz")
    if T == 1 or case == "n257":
        # one tracer without the tracer axis, both outputs skipped
        f1 = to_dev(np.asfortranarray(f[..., 0]))
        wp = SM.make_wp(ncrms, nx, nz, None, dt, 650)
        M.sediment(f1, to_dev(rho), to_dev(adz), to_dev(wp))
        torch.cuda.synchronize()
        assert_bitwise(to_host(f1), SM.sediment(f[..., 0], rho, adz, wp)[0], f"array form {case}, one tracer: f")


# ---- 4. every error code, in the stated order; the plan's state before and after
def test_errors_change_nothing(mpdata, oracle):
    M = mpdata
    name = "f64-nz28-nx11"
    shape, T, dt, _ = KINDS[name]
    ncrms, nx, nz = shape
    inp = inputs(oracle, name)
    w = to_dev(wp_of(name, 30))

    def code(fn, *a, **kw):
        with pytest.raises(M.MpdataError) as e:
            fn(*a, **kw)
        return e.value.code

    p = new_plan(M, name)
    assert code(p.sediment, w) == M.ESTATE                                       # never filled
    upload(p, inp)
    before = whole(M, p, name)
    L = M.lib()
    raw = lambda sl0, n, first, ntr, wp=w.data_ptr(): L.mpdata_plan_sediment_device(p._p, sl0, n, wp, None, None, first, ntr)
    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, ncrms + 1), (ncrms, 1), (3, 3)):
        assert raw(sl0, n, 0, 1) == M.EINVAL, (sl0, n)
    for first, ntr in ((0, 0), (-1, 1), (1, 2), (2, 1), (0, 3)):
        assert raw(0, ncrms, first, ntr) == M.EINVAL, (first, ntr)
    assert raw(0, ncrms, 0, 1, None) == M.EINVAL and b"null wp" in L.mpdata_last_error()
    assert raw(0, 0, 0, 1, None) == M.EINVAL and b"n = 0" in L.mpdata_last_error()                # the range first
    assert raw(0, ncrms, 0, 3, None) == M.EINVAL and b"tracer range" in L.mpdata_last_error()     # then the tracers
    # a host form of the other precision; its NULL comes first
    w32 = np.asfortranarray(wp_of(name, 30).astype(F32))
    assert L.mpdata_plan_sediment_f32(p._p, 0, ncrms, w32.ctypes.data, None, None) == M.ESTATE
    assert L.mpdata_plan_sediment_f32(p._p, 0, ncrms, None, None, None) == M.EINVAL and b"null wp" in L.mpdata_last_error()
    # the array forms: sizes, the block, f, rho, adz, then wp
    one = 8
    arr = L.mpdata_sediment_device
    assert arr(4, 5, 1, 1, 0, 4, None, None, None, None, None, None, None) == M.EINVAL and b"nz=1" in L.mpdata_last_error()
    assert arr(4, 5, 6, 1, 2, 3, None, None, None, None, None, None, None) == M.EINVAL and b"outside" in L.mpdata_last_error()
    for i, nm in enumerate(("f", "rho", "adz", "wp")):
        args = [one] * 4
        args[i] = None
        assert arr(4, 5, 6, 1, 0, 4, *args, None, None, None) == M.EINVAL and b"null " + nm.encode() in L.mpdata_last_error(), nm
    assert arr(4, 5, 6, 1, 0, 4, None, None, None, None, None, None, None) == M.EINVAL and b"null f" in L.mpdata_last_error()
    after = whole(M, p, name)
    for k in before:
        assert_bitwise(after[k], before[k], f"after the refused calls: {k}")
    p.sediment(w)                                                                # ... and the plan still works
    p.sync()
    assert not np.array_equal(whole(M, p, name, ("f",))["f"], before["f"])
    p.close()


# ---- 5. a multi-GPU handle is refused; the single-device plans of its shards take the call
def test_multi_gpu_handle_and_shard_plan(mpdata, oracle, monkeypatch):
    M = mpdata
    monkeypatch.delenv("MPDATA_MULTI_XFER", raising=False)
    name = "f64-nz28-nx11"
    shape, T, dt, _ = KINDS[name]
    ncrms, nx, nz = shape
    inp = inputs(oracle, name)
    p = M.Plan(*shape, T, dtype=dt, devices=[0, 0])
    upload(p, inp)
    m = model_of(oracle, name)
    w = wp_of(name, 40)
    with pytest.raises(M.MpdataError) as e:
        p.sediment(to_dev(w))
    assert e.value.code == M.EUNSUPPORTED and b"mpdata_plan_shard_plan" in M.lib().mpdata_last_error()
    with pytest.raises(M.MpdataError) as e:
        p.sediment_host(w)
    assert e.value.code == M.EUNSUPPORTED
    same_as_model(M, p, name, m, "after the refused handle calls")
    for g, (_, s0, nloc) in enumerate(p.shards()):
        q = p.shard_plan(g)
        wg = wp_of(name, 41 + g, nloc)
        got = sediment(M, q, name, wg, 0, nloc)
        check_outs(got, m.sediment(wg, sl0=s0, n=nloc), f"shard {g}")
        q.close()
    same_as_model(M, p, name, m, "after the shard plans' calls")
    p.run()
    assert m.run() is None
    same_as_model(M, p, name, m, "after the shard plans' calls and a run")
    p.close()


# ---- 6. the Fortran program: every record of its dump against the model
FORTRAN = {
    "f64": (F64, "sediment_calls", (7, 5, 10), 3, (2, 3), (1, 2)), "f32": (F32, "sediment_calls_sp", (6, 5, 10), 3, (1, 3), (1, 2)),
    "f64-whole": (F64, "sediment_calls", (5, 3, 28), 2, (0, 5), (0, 2)), "f32-odd-ref": (F32, "sediment_calls_sp", (7, 3, 12), 2, (6, 1), (1, 1)),
    "f64-nz72": (F64, "sediment_calls", (3, 2, 72), 1, (1, 2), (0, 1)), "f32-nz72": (F32, "sediment_calls_sp", (4, 2, 72), 2, (1, 2), (0, 2)),
}


@pytest.mark.parametrize("case", list(FORTRAN))
def test_fortran_program_matches_the_model(oracle, tmp_path, case):
    dt, exe, shape, T, (sl0, n), (t1, tn) = FORTRAN[case]
    ncrms, nx, nz = shape
    inp = SM.make_plan_inputs(oracle, shape, T, dt, SEED + 3)
    arrs = {k: (inp[k].reshape(inp[k].shape + (1,), order="F") if T == 1 and k in ("f", "flux") else inp[k]) for k in PM.NAMES}
    wp_a = SM.make_wp(n, nx, nz, T, dt, 700)
    wp_b = SM.make_wp(ncrms, nx, nz, tn, dt, 701)
    records = [("params", np.array([ncrms, nx, nz, T, sl0, n, t1, tn], np.int64))]
    records += [(k, arrs[k]) for k in PM.NAMES] + [("wp_a", wp_a), ("wp_b", wp_b)]
    # the replay on the model
    m = SM.PlanModelSediment(oracle, ncrms, nx, nz, T, dt)
    want = FR.want_import(m, inp)
    rc = lambda what, code=None: want.append(FR.rc(what, code))
    psfc, pflux = m.sediment(wp_a, sl0=sl0, n=n)
    rc("sed_block"); rc("sync")
    want += [("psfc", psfc), ("pflux", pflux)]
    assert m.sediment(wp_b, first=t1, ntr=tn) is not None
    rc("sed_range"); rc("sync")
    want += FR.want_close(m)
    FR.compare_dump(FR.run_program(exe, records, tmp_path), want, case)
