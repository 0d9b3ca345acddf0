"""GPU tests of the eddy diffusion of a resident plan (include/mpdata_hip.h 3l): mpdata_plan_diffuse_device, the host
forms, the array forms and their Python face Plan.diffuse / diffuse_host / diffuse.

Every comparison is bit for bit (util.assert_bitwise) against the numpy model of tests/diffuse_model.py: DM.diffuse on a
reference-layout truth, or the plan model with the new call (DM.PlanModelDiffuse: oracle/plan_model.py; an EXACT plan's f
and flux are bit-identical to it), or, for FAST plans, the plan's own whole export before the call.  zflux lies inside a
larger buffer with a patterned band of 4 KiB on both sides; the bands must come back unchanged, and so must the inputs.

Shapes: the smallest at which each path of the kernel differs.  nx = 8 is one full batch of columns, nx = 3 a cut one,
nx = 11 a full and a cut one.  ncrms 3 and 5 leave padding in the last tile; 34 instances at nz = 6 are five tiles of
eight, a second workgroup of the plan-layout kernel (it owns four one-slice tiles).  nz = 6: eight lanes per instance;
28: 32 lanes, the chunk has a line-aligned part and a rest; 33: one instance per wave (the threshold of the packed fp32
forms); 64 and 65: 63 and 64 elements, the last lane's upper neighbour; 72, 130 and 200: an instance is two, three and four
64-element slices of one tile, its vertical neighbours cross waves (three slices: the fourth wave idles)."""
import numpy as np
import pytest

import diffuse_model as DM
import plan_harness as H
from oracle import plan_model as PM
from plan_harness import BAND, _defaults, banded, tdt, upload
from util import assert_bitwise, to_dev, to_host

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32

# name -> (shape, tracers, dtype, switches)
KINDS = {
    "f64-nz6": ((3, 8, 6), 2, F64, {}), "f64-nz6-n34": ((34, 8, 6), 1, F64, {}), "f64-nz28": ((5, 8, 28), 2, F64, {}),
    "f64-nz28-nx3": ((5, 3, 28), 1, F64, {}), "f64-nz28-nx11": ((3, 11, 28), 1, F64, {}), "f64-nz33": ((3, 8, 33), 1, F64, {}),
    "f64-nz64": ((3, 8, 64), 1, F64, {}), "f64-nz65": ((3, 8, 65), 1, F64, {}), "f64-nz72": ((3, 8, 72), 2, F64, {}),
    "f64-nz130": ((3, 8, 130), 1, F64, {}), "f64-nz200": ((3, 8, 200), 1, F64, {}),
    "f32-nz6-n34": ((34, 8, 6), 1, F32, {}), "f32-nz28-even": ((6, 8, 28), 2, F32, {}), "f32-nz33-even": ((4, 8, 33), 1, F32, {}),
    "f32-nz72-even": ((4, 8, 72), 1, F32, {}), "f32-nz130-even": ((4, 8, 130), 1, F32, {}),
    "f32-nz6-odd": ((5, 8, 6), 1, F32, dict(odd=True)), "f32-nz28-odd": ((5, 8, 28), 2, F32, dict(odd=True)),
    "f32-nz33-odd": ((3, 8, 33), 1, F32, dict(odd=True)), "f32-nz72-odd": ((3, 8, 72), 1, F32, dict(odd=True)),
    "f64-nz12-ref": ((5, 8, 12), 2, F64, dict(ref=True)), "f32-nz12-ref": ((5, 8, 12), 2, F32, dict(ref=True)),
    "f32-nz12-odd-ref": ((5, 8, 12), 1, F32, {}),      # (an odd fp32 plan without the switch keeps the reference layout)
}
SEED = 100


_INPUTS = {}


def inputs(oracle, name):
    """the seven arrays of KINDS[name]: computed once and shared; no test writes them"""
    if name not in _INPUTS:
        shape, T, dt, _ = KINDS[name]
        _INPUTS[name] = DM.make_plan_inputs(oracle, shape, T, dt, SEED)
    return _INPUTS[name]


def new_plan(M, name, variant=None):
    # (the layout from the name too: an odd fp32 plan without the opt-in lands in the reference layout; windows: not asserted)
    ref = bool(KINDS[name][3].get("ref")) or name.endswith("-odd-ref")
    return H.new_plan(M, KINDS[name], name, ref, None, variant)


def model_of(oracle, name):
    shape, T, dt, _ = KINDS[name]
    m = DM.PlanModelDiffuse(oracle, *shape, T, dt)
    assert m.upload({k: np.array(v, order="F") for k, v in inputs(oracle, name).items()}) is None
    return m


def whole(M, p, name, what=("f", "flux")):
    return H.whole(M, p, KINDS[name], what)


def same_as_model(M, p, name, m, what):
    H.same_as_model(M, p, KINDS[name], name, m, what)


def coeffs(name, k, n=None, fluxes=True):
    shape, T, dt, _ = KINDS[name]
    return DM.make_coeffs(shape[0] if n is None else n, shape[1], shape[2], dt, 500 + k, fluxes)


def diffuse(M, p, name, c, sl0=0, n=None, first=0, ntr=None, zflux=True, lead=None):
    """Plan.diffuse of host coefficients c -> zflux (n, nz, ntr) or None; the inputs and the bands of zflux are checked"""
    import torch
    shape, T, dt, _ = KINDS[name]
    n = shape[0] - sl0 if n is None else n
    ntr = T - first if ntr is None else ntr
    dev = {k: None if v is None else to_dev(v) for k, v in c.items()}
    orig = {k: None if v is None else v.clone() for k, v in dev.items()}
    lead = (ntr != 1) if lead is None else lead
    zb = banded(((ntr,) if lead else ()) + (shape[2], n), dt) if zflux else None
    torch.cuda.synchronize()      # (the plan may run on a stream that does not wait for the one that filled the buffers)
    p.diffuse(dev["tkh"], dev["cx"], dev["cz"], dev["sb"], dev["st"], zb[2] if zflux else None, sl0, n, first, ntr)
    p.sync()
    for k, v in dev.items():
        assert v is None or torch.equal(v, orig[k]), f"{k} changed"
    if not zflux:
        return None
    raw, pristine, view = zb
    assert torch.equal(raw[:BAND], pristine[:BAND]) and torch.equal(raw[-BAND:], pristine[-BAND:]), "zflux: a band byte changed"
    return to_host(view).reshape((n, shape[2], ntr), order="F")


# ---- 1. every kind of plan: whole plan, every state
@pytest.mark.parametrize("name", list(KINDS))
def test_every_plan_kind(mpdata, oracle, name):
    M = mpdata
    shape, T, dt, sw = KINDS[name]
    inp = inputs(oracle, name)
    p = new_plan(M, name)
    upload(p, inp)
    m = model_of(oracle, name)
    # (a) upload -> diffuse with sb, st, zflux -> the model on the uploaded f (its halo columns differ from the interior)
    c0 = coeffs(name, 0)
    assert not np.array_equal(inp["f"][:, 2], inp["f"][:, 3])
    z = diffuse(M, p, name, c0)
    want_f, want_z = DM.diffuse(inp["f"], inp["rho"], inp["adz"], **c0)
    assert_bitwise(z, want_z.reshape(z.shape, order="F"), f"{name} (a): zflux")
    assert_bitwise(z, m.diffuse(**c0), f"{name} (a): zflux of the plan model")
    got = whole(M, p, name)
    assert_bitwise(got["f"].reshape(want_f.shape, order="F"), want_f, f"{name} (a): f")
    assert_bitwise(got["flux"].reshape(inp["flux"].shape, order="F"), inp["flux"], f"{name} (a): flux")
    # (b) a run on the kept velocities = export -> model -> import -> run
    p.run()
    assert m.run() is None
    same_as_model(M, p, name, m, "(b) diffuse, run")
    # (c) PERIODIC: run, diffuse while the halos are stale (no fluxes, no zflux), export = the model after a wrap
    p.set_boundary(M.BOUNDARY_PERIODIC)
    assert m.set_boundary(PM.PERIODIC) is None
    p.run()
    assert m.run() is None
    c1 = coeffs(name, 1, fluxes=False)
    assert diffuse(M, p, name, c1, zflux=False) is None
    assert m.diffuse(**c1) is not None
    same_as_model(M, p, name, m, "(c) periodic: run, diffuse on stale halos")
    # ... and once more on the halos that export wrapped; only one of sb, st; then a run
    c2 = dict(coeffs(name, 2), st=None)
    z = diffuse(M, p, name, c2)
    assert_bitwise(z, m.diffuse(**c2), f"{name} (c) periodic, fresh halos: zflux")
    p.run()
    assert m.run() is None
    same_as_model(M, p, name, m, "(c) periodic: diffuse on fresh halos, run")
    # (d) GIVEN again, run_uw (the plan holds no velocities afterwards), diffuse with st alone
    p.set_boundary(M.BOUNDARY_GIVEN)
    assert m.set_boundary(PM.GIVEN) is None
    other = DM.make_plan_inputs(oracle, shape, T, dt, SEED + 50)
    p.run_uw(to_dev(other["u"]), to_dev(other["w"]))
    assert m.run_uw(other["u"], other["w"]) is None
    c3 = dict(coeffs(name, 3), sb=None)
    z = diffuse(M, p, name, c3)
    assert_bitwise(z, m.diffuse(**c3), f"{name} (d) run_uw, diffuse: zflux")
    same_as_model(M, p, name, m, "(d) run_uw, diffuse")
    p.close()
    # FAST: the same bits as EXACT on the uploaded f; after a run against the plan's own export changed by the model
    p = new_plan(M, name, variant=M.VARIANT_FAST)
    upload(p, inp)
    z = diffuse(M, p, name, c0)
    assert_bitwise(z, want_z.reshape(z.shape, order="F"), f"{name} FAST: zflux")
    assert_bitwise(whole(M, p, name, ("f",))["f"].reshape(want_f.shape, order="F"), want_f, f"{name} FAST upload, diffuse")
    p.run()
    E = whole(M, p, name, ("f",))["f"].reshape(want_f.shape, order="F")
    diffuse(M, p, name, c1, zflux=False)
    got = whole(M, p, name, ("f",))["f"].reshape(want_f.shape, order="F")
    assert_bitwise(got, DM.diffuse(E, inp["rho"], inp["adz"], **c1)[0], f"{name} FAST run, diffuse")
    p.close()


# ---- 2. blocks and tracer sub-ranges: what lies outside keeps every bit
BLOCKS = {
    # eight instances per tile: inside the first tile, across two tiles from mid-tile, the last tile's two, one from a boundary
    "f64-nz6-n34": [(1, 3), (5, 14), (32, 2), (8, 1), (0, 34)],
    # two per tile: mid-tile to mid-tile, the last (half-filled) tile
    "f64-nz28": [(1, 3), (4, 1), (0, 4)],
    "f64-nz72": [(1, 1), (1, 2)],
    # fp32, 16 per tile: blocks that split pairs at both ends, inside one tile and across tiles
    "f32-nz6-n34": [(1, 2), (15, 4), (3, 30), (33, 1)],
    # fp32 pairs, odd plan of 5 (4 per tile; instance 4 shares its pair with the phantom): a split pair, blocks that hold
    # and miss instance ncrms - 1, one that ends inside the first tile
    "f32-nz28-odd": [(1, 2), (4, 1), (3, 2), (0, 4), (0, 3), (0, 5)],
    "f32-nz72-odd": [(2, 1), (1, 1), (0, 2)],
    "f32-nz130-even": [(1, 2), (3, 1)],
    "f64-nz12-ref": [(1, 3), (4, 1)],
    "f32-nz12-ref": [(1, 3)],
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
        c = coeffs(name, 10 + k, n)
        z = diffuse(M, p, name, c, sl0, n, first, ntr, lead=bool(k % 2) or ntr > 1)
        want_z = m.diffuse(**c, sl0=sl0, n=n, first=first, ntr=ntr)
        assert_bitwise(z, want_z, f"{name} block {sl0, n} tracers {first, ntr}: zflux")
        after = whole(M, p, name)
        out = np.ones(ncrms, bool)
        out[sl0:sl0 + n] = False
        tout = np.ones(T, bool)
        tout[first:first + ntr] = False
        assert_bitwise(after["f"][out], before["f"][out], f"{name} block {sl0, n}: instances outside")
        assert_bitwise(after["f"][..., tout], before["f"][..., tout], f"{name} block {sl0, n}: tracers outside")
        assert_bitwise(after["flux"], before["flux"], f"{name} block {sl0, n}: flux")
        want = DM.diffuse(before["f"][sl0:sl0 + n, ..., first:first + ntr], inp["rho"][sl0:sl0 + n], inp["adz"][sl0:sl0 + n], **c)[0]
        assert_bitwise(after["f"][sl0:sl0 + n, ..., first:first + ntr], want, f"{name} block {sl0, n}: inside")
        assert not np.array_equal(want, before["f"][sl0:sl0 + n, ..., first:first + ntr])
        # a run of every instance (the phantom of an odd plan rides with instance ncrms - 1) matches the model
        p.run()
        assert m.run() is None
        same_as_model(M, p, name, m, f"block {sl0, n}, run")
    p.close()


# ---- 3. the host form and the array forms
@pytest.mark.parametrize("name", ["f64-nz28", "f32-nz28-odd", "f64-nz12-ref", "f64-nz72"])
def test_host_form(mpdata, oracle, name):
    M = mpdata
    shape, T, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    inp = inputs(oracle, name)
    p = new_plan(M, name)
    upload(p, inp)
    m = model_of(oracle, name)
    for sl0, n, fl, wz in ((0, ncrms, True, True), (1, 2, False, False), (ncrms - 1, 1, True, True)):
        c = coeffs(name, 20 + sl0, n, fluxes=fl)
        z = np.full((n, nz) + ((T,) if T > 1 else ()), -7, dt, order="F") if wz else None
        p.diffuse_host(c["tkh"], c["cx"], c["cz"], c["sb"], c["st"], z, sl0, n)
        want_z = m.diffuse(**c, sl0=sl0, n=n)
        if wz:
            assert_bitwise(z.reshape(want_z.shape, order="F"), want_z, f"{name} host {sl0, n}: zflux")
        same_as_model(M, p, name, m, f"host form {sl0, n}")
    with pytest.raises(M.MpdataError):
        p.diffuse_host(c["tkh"][:, :-1], c["cx"], c["cz"], sl0=ncrms - 1, n=1)       # a wrong shape
    p.close()


@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
def test_array_forms(mpdata, oracle, dt):
    import torch
    M = mpdata
    shape, T = (7, 8, 6), 2
    ncrms, nx, nz = shape
    inp = DM.make_plan_inputs(oracle, shape, T, dt, SEED + 7)
    for sl0, n, fl, wz in ((0, 7, True, True), (2, 4, False, True), (6, 1, True, False)):
        c = DM.make_coeffs(n, nx, nz, dt, 600 + sl0, fluxes=fl)
        f = to_dev(inp["f"])
        dev = {k: None if v is None else to_dev(v) for k, v in c.items()}
        zb = banded((T, nz, n), dt) if wz else None
        torch.cuda.synchronize()
        M.diffuse(f, to_dev(inp["rho"]), to_dev(inp["adz"]), dev["tkh"], dev["cx"], dev["cz"], dev["sb"], dev["st"],
                  zb[2] if wz else None, sl0, n)
        torch.cuda.synchronize()
        got = to_host(f)
        want, want_z = DM.diffuse(inp["f"][sl0:sl0 + n], inp["rho"][sl0:sl0 + n], inp["adz"][sl0:sl0 + n], **c)
        out = np.ones(ncrms, bool)
        out[sl0:sl0 + n] = False
        assert_bitwise(got[sl0:sl0 + n], want, f"array form {sl0, n}: inside")
        assert_bitwise(got[out], inp["f"][out], f"array form {sl0, n}: outside")
        if wz:
            raw, pristine, view = zb
            assert torch.equal(raw[:BAND], pristine[:BAND]) and torch.equal(raw[-BAND:], pristine[-BAND:])
            assert_bitwise(to_host(view), want_z, f"array form {sl0, n}: zflux")
    # one tracer without the tracer axis
    f1 = to_dev(np.asfortranarray(inp["f"][..., 0]))
    c = DM.make_coeffs(ncrms, nx, nz, dt, 610)
    dev = {k: to_dev(v) for k, v in c.items()}
    z1 = torch.empty((nz, ncrms), dtype=tdt(dt), device="cuda:0")
    M.diffuse(f1, to_dev(inp["rho"]), to_dev(inp["adz"]), dev["tkh"], dev["cx"], dev["cz"], dev["sb"], dev["st"], z1)
    torch.cuda.synchronize()
    want, want_z = DM.diffuse(inp["f"][..., 0], inp["rho"], inp["adz"], **c)
    assert_bitwise(to_host(f1), want, "array form, one tracer: f")
    assert_bitwise(to_host(z1), want_z, "array form, one tracer: zflux")


# ---- 4. every error code; the plan's state before and after
def test_errors_change_nothing(mpdata, oracle):
    import torch
    M = mpdata
    name = "f64-nz28"
    shape, T, dt, _ = KINDS[name]
    ncrms, nx, nz = shape
    inp = inputs(oracle, name)
    c = coeffs(name, 30)
    dev = {k: to_dev(v) for k, v in c.items()}
    args = (dev["tkh"], dev["cx"], dev["cz"], dev["sb"], dev["st"])

    def code(fn, *a, **kw):
        with pytest.raises(M.MpdataError) as e:
            fn(*a, **kw)
        return e.value.code

    p = new_plan(M, name)
    assert code(p.diffuse, *args) == M.ESTATE                                   # never filled
    upload(p, inp)
    p.set_boundary(M.BOUNDARY_PERIODIC)
    p.run()                                                                      # (stale halos: a failed call must not wrap)
    p.set_boundary(M.BOUNDARY_GIVEN)
    before = whole(M, p, name)
    L = M.lib()
    ptr = {k: v.data_ptr() for k, v in dev.items()}
    raw = lambda sl0, n, first, ntr, **kw: L.mpdata_plan_diffuse_device(
        p._p, sl0, n, *[kw.get(k, ptr[k]) for k in ("tkh", "cx", "cz", "sb", "st")], None, first, ntr)
    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, ncrms + 1), (ncrms, 1), (3, 3)):
        assert raw(sl0, n, 0, 1) == M.EINVAL, (sl0, n)
    for first, ntr in ((0, 0), (-1, 1), (1, 2), (2, 1), (0, 3)):
        assert raw(0, ncrms, first, ntr) == M.EINVAL, (first, ntr)
    for k in ("tkh", "cx", "cz"):
        assert raw(0, ncrms, 0, 1, **{k: None}) == M.EINVAL, k
        assert b"null " + k.encode() in L.mpdata_last_error()
    assert raw(0, 0, 0, 1, tkh=None) == M.EINVAL and b"n = 0" in L.mpdata_last_error()          # the range first
    # a host form of the other precision
    c32 = {k: np.asfortranarray(v.astype(F32)) for k, v in c.items()}
    rc = L.mpdata_plan_diffuse_f32(p._p, 0, ncrms, *[c32[k].ctypes.data for k in ("tkh", "cx", "cz", "sb", "st")], None)
    assert rc == M.ESTATE
    after = whole(M, p, name)
    for k in before:
        assert_bitwise(after[k], before[k], f"after the refused calls: {k}")
    assert p.boundary == M.BOUNDARY_GIVEN
    p.diffuse(*args)                                                             # ... and the plan still works
    p.sync()
    assert not np.array_equal(whole(M, p, name, ("f",))["f"], before["f"])
    p.close()
    # a windowed plan: not built yet
    M.set_tall_columns(1)
    pw = M.Plan(2, 8, 250, 1)
    assert pw.level_windows > 1
    iw = DM.make_plan_inputs(oracle, (2, 8, 250), 1, F64, SEED)
    upload(pw, iw)
    cw = DM.make_coeffs(2, 8, 250, F64, 31)
    dw = {k: to_dev(v) for k, v in cw.items()}
    fw = torch.empty(M.shapes(2, 8, 250, 1)["f"], dtype=torch.float64, device="cuda:0")
    pw.export_device(f=fw)
    pw.sync()
    assert code(pw.diffuse, dw["tkh"], dw["cx"], dw["cz"]) == M.EUNSUPPORTED
    assert b"windowed" in L.mpdata_last_error()
    assert code(pw.diffuse, dw["tkh"], dw["cx"], dw["cz"], sl0=0, n=3) == M.EINVAL           # the range comes first
    fw2 = torch.empty_like(fw)
    pw.export_device(f=fw2)
    pw.sync()
    assert torch.equal(fw.view(torch.int64), fw2.view(torch.int64))
    pw.close()


# ---- 5. a multi-GPU handle is refused; the single-device plans of its shards take the call
def test_multi_gpu_handle_and_shard_plan(mpdata, oracle, monkeypatch):
    M = mpdata
    monkeypatch.delenv("MPDATA_MULTI_XFER", raising=False)
    name = "f64-nz28"
    shape, T, dt, _ = KINDS[name]
    inp = inputs(oracle, name)
    p = M.Plan(*shape, T, dtype=dt, devices=[0, 0])
    upload(p, inp)
    m = model_of(oracle, name)
    c = coeffs(name, 40)
    dev = {k: to_dev(v) for k, v in c.items()}
    with pytest.raises(M.MpdataError) as e:
        p.diffuse(dev["tkh"], dev["cx"], dev["cz"], dev["sb"], dev["st"])
    assert e.value.code == M.EUNSUPPORTED and b"mpdata_plan_shard_plan" in M.lib().mpdata_last_error()
    with pytest.raises(M.MpdataError) as e:
        p.diffuse_host(c["tkh"], c["cx"], c["cz"])
    assert e.value.code == M.EUNSUPPORTED
    same_as_model(M, p, name, m, "after the refused handle calls")
    for g, (_, s0, nloc) in enumerate(p.shards()):
        q = p.shard_plan(g)
        cg = coeffs(name, 41 + g, nloc)
        z = diffuse(M, q, name, cg, 0, nloc)
        assert_bitwise(z, m.diffuse(**cg, sl0=s0, n=nloc), f"shard {g}: zflux")
        q.close()
    same_as_model(M, p, name, m, "after the shard plans' diffusions")
    p.run()
    assert m.run() is None
    same_as_model(M, p, name, m, "after the shard plans' diffusions and a run")
    p.close()
