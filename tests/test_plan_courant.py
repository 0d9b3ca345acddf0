"""GPU tests of the outflow Courant number of a plan's velocities (include/mpdata_hip.h 3h): mpdata_plan_courant_device,
the host forms, the array forms and their Python face Plan.courant / courant_host / courant.

Every comparison is bit for bit (util.assert_bitwise) against the numpy model of tests/courant_model.py -- the definition
statement by statement in the arrays' dtype -- applied to the reference-layout arrays that were uploaded or imported.
Every device output lies inside a larger buffer with a patterned band of 4 KiB on both sides that must come back unchanged.
The inputs are those of tests/level_stats_model.py (shapes) as tests/courant_model.py makes them (signed velocities, a
w(:, :, nz) that is nowhere zero, rho and adz that vary along the column); tests/test_courant_cpu.py holds the guard that
every named wrong variant shows on each of them."""
import ctypes

import numpy as np
import pytest

import courant_model as CM
import level_stats_model as LM
from plan_harness import BAND, _defaults, banded, tdt, upload
from test_plan_level_stats import chunk_kind, new_plan
from util import assert_bitwise, to_dev, to_host

pytestmark = pytest.mark.gpu


BOTH = ("clev", "cinst")


def cour(p, dt, nzm, sl0, n, which=BOTH):
    """Plan.courant into banded buffers -> {name: clev (n, nzm) Fortran array / cinst (n,)}; the bands are checked"""
    import torch
    bufs = {k: banded((nzm, n) if k == "clev" else (n,), dt) for k in which}
    torch.cuda.synchronize()      # (the plan may run on a stream that does not wait for the one that filled the buffers)
    p.courant(sl0, n, **{k: v[2] for k, v in bufs.items()})
    p.sync()
    out = {}
    for k, (raw, orig, view) in bufs.items():
        assert torch.equal(raw[:BAND], orig[:BAND]) and torch.equal(raw[-BAND:], orig[-BAND:]), f"{k}: a band byte changed"
        out[k] = to_host(view)
    return out


def model(u, w, rho, adz, sl0=0, n=None):
    clev, cinst = CM.courant(u, w, rho, adz)
    n = clev.shape[0] - sl0 if n is None else n
    return {"clev": np.asfortranarray(clev[sl0:sl0 + n]), "cinst": np.ascontiguousarray(cinst[sl0:sl0 + n])}


def same(got, want, what):
    for k in got:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k, got[k].shape, want[k].shape)
        assert_bitwise(got[k], want[k], f"{what}: {k}")


def check_whole(p, name, u, w, inp, what):
    shape, _, dt, _ = LM.INPUTS[name]
    same(cour(p, dt, shape[2] - 1, 0, shape[0]), model(u, w, inp["rho"], inp["adz"]), f"{name} {what}")


def code(M, fn, *a, **kw):
    with pytest.raises(M.MpdataError) as e:
        fn(*a, **kw)
    return e.value.code


# ---- 1. every kind of plan, every state
KINDS = [(f"f64-nz{nz}", {}, chunk_kind(nz)) for nz in (3, 5, 12, 28, 58, 72, 130)] + \
        [(f"f64-nx{nx}", {}, "") for nx in (1, 2, 5, 32)] + \
        [(f"f32-nz{nz}-even", {}, chunk_kind(nz, np.float32)) for nz in (5, 28, 72)] + \
        [(f"f32-nz{nz}-odd", dict(odd=True), "phantom") for nz in (5, 28, 72)] + \
        [("f32-nz12-odd-ref", {}, "reference-layout"), ("f64-nz12-ref", dict(ref=True), ""), ("f32-nz12-ref", dict(ref=True), ""),
         ("f64-tall", dict(tall=True), "windowed"), ("f32-tall-odd", dict(tall=True, odd=True), "windowed-phantom"),
         ("f64-tall-kmarch", {}, "reference-layout")]


@pytest.mark.parametrize("name,sw,note", KINDS, ids=[f"{k}{'-' + n if n else ''}" for k, _, n in KINDS])
def test_every_plan_kind_and_state(mpdata, oracle, name, sw, note):
    import torch
    M = mpdata
    shape, T, dt, _ = LM.INPUTS[name]
    ncrms, nx, nz = shape
    inp = CM.make(oracle, name)
    p = new_plan(M, name, **sw)
    want_layout = M.LAYOUT_REFERENCE if (sw.get("ref") or "reference-layout" in note) else M.LAYOUT_WAVEMAJOR
    assert p.layout == want_layout and (p.level_windows > 1) == bool(sw.get("tall"))
    out = torch.zeros((ncrms,), dtype=tdt(dt), device="cuda:0")
    assert code(M, p.courant, 0, ncrms, cinst=out) == M.ESTATE                # never filled
    assert code(M, p.courant_host, 0, ncrms) == M.ESTATE
    upload(p, inp)
    u, w = inp["u"], inp["w"]
    check_whole(p, name, u, w, inp, "after the upload")
    # a run: the same result, and the run's event pair is not touched
    p.run()
    p.sync()
    ms = p.last_kernel_ms()
    check_whole(p, name, u, w, inp, "after a run")
    assert p.last_kernel_ms() == ms
    p.run()                                                                  # (the plan still holds u and w)
    # a whole import of new u, w
    u2, w2 = CM.other(oracle, name, 50)
    p.import_device(u=to_dev(u2), w=to_dev(w2))
    check_whole(p, name, u2, w2, inp, "after a whole import of u, w")
    # a block import of u and w that replaces the plan's last instance
    u3, w3 = np.array(u2, order="F"), np.array(w2, order="F")
    u3[ncrms - 1:], w3[ncrms - 1:] = u[ncrms - 1:], w[ncrms - 1:]
    p.import_block(ncrms - 1, u=to_dev(np.asfortranarray(u[ncrms - 1:])), w=to_dev(np.asfortranarray(w[ncrms - 1:])))
    check_whole(p, name, u3, w3, inp, "after a block import of the last instance")
    # run_uw uses the plan's velocities up: a state error until BOTH have been imported again
    u4, w4 = CM.other(oracle, name, 77)
    p.run_uw(to_dev(u4), to_dev(w4))
    assert code(M, p.courant, 0, ncrms, cinst=out) == M.ESTATE
    assert code(M, p.courant_host, 0, ncrms) == M.ESTATE
    p.import_device(u=to_dev(u4))
    assert code(M, p.courant, 0, ncrms, cinst=out) == M.ESTATE
    assert b"does not hold w" in M.lib().mpdata_last_error()
    p.import_device(w=to_dev(w4))
    check_whole(p, name, u4, w4, inp, "after run_uw and an import of u, then w")
    p.sync()
    assert not out.any()                                                      # (no refused call wrote)
    p.close()
    # FAST plans: the same bits
    p = new_plan(M, name, variant=M.VARIANT_FAST, **sw)
    upload(p, inp)
    check_whole(p, name, u, w, inp, "FAST after the upload")
    p.close()


# ---- 2. a PERIODIC plan; and the calls change nothing a later run can see (halo and seam marks, the velocities)
@pytest.mark.parametrize("name,sw", [("f64-nz28", {}), ("f32-nz28-odd", dict(odd=True)), ("f64-tall", dict(tall=True)),
                                     ("f64-nz12-ref", dict(ref=True))], ids=lambda v: v if isinstance(v, str) else "")
def test_periodic_plan_and_no_state_change(mpdata, oracle, name, sw):
    import torch
    M = mpdata
    shape, T, dt, _ = LM.INPUTS[name]
    ncrms, nx, nz = shape
    inp = CM.make(oracle, name)
    for k in ("u", "w"):       # velocities of a size the scheme is stable at (a power of two: the model sees the same arrays)
        inp[k] = np.asfortranarray(inp[k] * dt(2.0 ** -5))
    got = {}
    for with_calls in (False, True):
        p = new_plan(M, name, **sw)
        p.set_boundary(M.BOUNDARY_PERIODIC)
        upload(p, inp)
        for step in range(3):
            if with_calls:
                check_whole(p, name, inp["u"], inp["w"], inp, f"periodic, in front of run {step}")
                lev, ins = p.courant_host(1, 2)
                assert_bitwise(ins, model(inp["u"], inp["w"], inp["rho"], inp["adz"], 1, 2)["cinst"], "host form")
            p.run()
        f = torch.empty(M.shapes(*shape, T)["f"], dtype=tdt(dt), device="cuda:0")
        flux = torch.empty(M.shapes(*shape, T)["flux"], dtype=tdt(dt), device="cuda:0")
        p.export_device(f=f, flux=flux)
        p.sync()
        got[with_calls] = (to_host(f), to_host(flux))
        p.close()
    assert_bitwise(got[True][0], got[False][0], f"{name}: f after three periodic runs with and without the calls")
    assert_bitwise(got[True][1], got[False][1], f"{name}: flux after three periodic runs with and without the calls")


# ---- 3. blocks: n = 1, a block that splits a tile, one that splits an fp32 pair, one that ends at ncrms - 1; each with clev
# only, cinst only and both
BLOCKS = ((0, 11), (0, 1), (10, 1), (3, 5), (1, 9), (5, 6), (2, 8))


@pytest.mark.parametrize("name,sw", [("f64-blocks", {}), ("f32-blocks", dict(odd=True)), ("f64-tall-blocks", dict(tall=True)),
                                     ("f32-tall-blocks", dict(tall=True, odd=True)), ("f64-blocks", dict(ref=True))],
                         ids=["f64", "f32-odd", "f64-tall", "f32-tall-odd", "f64-ref"])
def test_blocks(mpdata, oracle, name, sw):
    M = mpdata
    shape, T, dt, _ = LM.INPUTS[name]
    ncrms, nx, nz = shape
    assert ncrms == 11
    inp = CM.make(oracle, name)
    p = new_plan(M, name, **sw)
    assert p.layout == (M.LAYOUT_REFERENCE if sw.get("ref") else M.LAYOUT_WAVEMAJOR)
    upload(p, inp)
    for sl0, n in BLOCKS:
        want = model(inp["u"], inp["w"], inp["rho"], inp["adz"], sl0, n)
        for which in (BOTH, ("clev",), ("cinst",)):
            got = cour(p, dt, nz - 1, sl0, n, which)
            assert set(got) == set(which)
            same(got, want, f"{name} block {sl0, n} {which}")
    p.close()


# ---- 4. signed zeros: +0.0 and -0.0 mixed in u, w give all-(+0.0) bits; and single non-zero faces among them
@pytest.mark.parametrize("name,sw", [("f64-nz28", {}), ("f32-nz28-odd", dict(odd=True)), ("f64-nz12-ref", dict(ref=True)),
                                     ("f32-tall-odd", dict(tall=True, odd=True))], ids=lambda v: v if isinstance(v, str) else "")
def test_signed_zeros(mpdata, oracle, name, sw):
    M = mpdata
    shape, T, dt, _ = LM.INPUTS[name]
    ncrms, nx, nz = shape
    inp = CM.make(oracle, name)
    rng = np.random.default_rng(11)
    inp["u"] = np.where(rng.random(inp["u"].shape) < 0.5, 0.0, -0.0).astype(dt, order="F")
    inp["w"] = np.where(rng.random(inp["w"].shape) < 0.5, 0.0, -0.0).astype(dt, order="F")
    inp["w"][:, :, -1] = 3.0                      # (never read)
    assert LM.has_negative_zero(inp["u"]) and LM.has_negative_zero(inp["w"])
    p = new_plan(M, name, **sw)
    upload(p, inp)
    got = cour(p, dt, nz - 1, 0, ncrms)
    assert not LM.bits(got["clev"]).any() and not LM.bits(got["cinst"]).any()
    u, w = np.array(inp["u"], order="F"), np.array(inp["w"], order="F")
    u[0, 3, 0], u[ncrms - 1, 2, nz - 2], w[1, 2, 1], w[ncrms - 1, nx + 1, nz - 2] = 0.5, -0.25, -0.125, 0.75
    p.import_device(u=to_dev(u), w=to_dev(w))
    want = model(u, w, inp["rho"], inp["adz"])
    assert np.count_nonzero(want["clev"]) >= 4
    same(cour(p, dt, nz - 1, 0, ncrms), want, f"{name} single faces among signed zeros")
    p.close()


# ---- 5. the host forms equal the device forms
@pytest.mark.parametrize("name,sw", [("f64-blocks", {}), ("f32-blocks", dict(odd=True)), ("f32-nz12-ref", dict(ref=True)),
                                     ("f64-tall", dict(tall=True))], ids=lambda v: v if isinstance(v, str) else "")
def test_host_forms(mpdata, oracle, name, sw):
    M = mpdata
    shape, T, dt, _ = LM.INPUTS[name]
    ncrms, nx, nz = shape
    inp = CM.make(oracle, name)
    p = new_plan(M, name, **sw)
    upload(p, inp)
    L = M.lib()
    fn = getattr(L, "mpdata_plan_courant" + ("" if dt == np.float64 else "_f32"))
    for sl0, n in ((0, ncrms), (1, ncrms - 2), (ncrms - 1, 1)):     # (the staging buffer grows and is reused)
        dev = cour(p, dt, nz - 1, sl0, n)
        lev, ins = p.courant_host(sl0, n)
        same({"clev": lev, "cinst": ins}, dev, f"{name} host {sl0, n}")
        same(dev, model(inp["u"], inp["w"], inp["rho"], inp["adz"], sl0, n), f"{name} device {sl0, n}")
        a = np.full((n, nz - 1), -7, dt, order="F")
        b = np.full((n,), -7, dt)
        assert fn(p._p, sl0, n, ctypes.c_void_p(a.ctypes.data), None) == 0
        assert fn(p._p, sl0, n, None, ctypes.c_void_p(b.ctypes.data)) == 0
        same({"clev": a, "cinst": b}, dev, f"{name} host, one output at a time {sl0, n}")
    # the form of the other precision
    z = np.zeros((ncrms, nz - 1), np.float32 if dt == np.float64 else np.float64, order="F")
    wrong = L.mpdata_plan_courant_f32 if dt == np.float64 else L.mpdata_plan_courant
    assert wrong(p._p, 0, ncrms, ctypes.c_void_p(z.ctypes.data), None) == M.ESTATE
    assert not z.any()
    assert fn(p._p, 0, ncrms, None, None) == M.EINVAL
    p.close()


# ---- 6. the array forms at an unaligned base, on a stream of their own; and array form == plan form on the same inputs
@pytest.mark.parametrize("name,sw", [("f64-array", {}), ("f32-array", dict(odd=True)), ("f64-nz28", {}), ("f32-nz72-odd", dict(odd=True))],
                         ids=lambda v: v if isinstance(v, str) else "")
def test_array_forms(mpdata, oracle, name, sw):
    import torch
    M = mpdata
    shape, T, dt, _ = LM.INPUTS[name]
    ncrms, nx, nz = shape
    inp = CM.make(oracle, name)
    want = model(inp["u"], inp["w"], inp["rho"], inp["adz"])
    isz = np.dtype(dt).itemsize

    def unaligned(a):   # the array one real behind a 256-byte boundary
        flat = torch.zeros(a.size + 1 + 256 // isz, dtype=tdt(dt), device="cuda:0")
        off = (-flat.data_ptr() // isz) % (256 // isz) + 1
        v = flat[off:off + a.size].view(tuple(reversed(a.shape)))
        v.copy_(to_dev(a))
        assert v.data_ptr() % 256 == isz
        return v
    d = {k: unaligned(inp[k]) for k in ("u", "w", "rho", "adz")}
    keep = {k: v.clone() for k, v in d.items()}
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    bufs = {"clev": banded((nz - 1, ncrms), dt), "cinst": banded((ncrms,), dt)}
    M.courant(d["u"], d["w"], d["rho"], d["adz"], stream=s, **{k: v[2] for k, v in bufs.items()})
    s.synchronize()
    same({k: to_host(v[2]) for k, v in bufs.items()}, want, name)
    for k, (raw, orig, _) in bufs.items():
        assert torch.equal(raw[:BAND], orig[:BAND]) and torch.equal(raw[-BAND:], orig[-BAND:]), k
    assert all(torch.equal(d[k], keep[k]) for k in d)
    for k in BOTH:                                          # the current stream, one output
        only = banded((nz - 1, ncrms) if k == "clev" else (ncrms,), dt)
        M.courant(d["u"], d["w"], d["rho"], d["adz"], **{k: only[2]})
        torch.cuda.synchronize()
        assert_bitwise(to_host(only[2]), want[k], f"{name} {k} alone")
        assert torch.equal(only[0][:BAND], only[1][:BAND]) and torch.equal(only[0][-BAND:], only[1][-BAND:])
    assert code(M, M.courant, d["u"], d["w"], d["rho"], d["adz"]) == -1
    # the plan form on the same inputs
    p = new_plan(M, name, **sw)
    upload(p, inp)
    same(cour(p, dt, nz - 1, 0, ncrms), {k: to_host(v[2]) for k, v in bufs.items()}, f"{name}: plan form against array form")
    p.close()


# ---- 7. errors
def test_errors(mpdata, oracle):
    import torch
    M = mpdata
    name = "f64-blocks"
    shape, T, dt, _ = LM.INPUTS[name]
    ncrms, nx, nz = shape
    p = new_plan(M, name)
    upload(p, CM.make(oracle, name))
    out = torch.zeros((nz - 1, ncrms), dtype=torch.float64, device="cuda:0")
    ptr = ctypes.c_void_p(out.data_ptr())
    L = M.lib()
    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, ncrms + 1), (ncrms, 1), (5, 7)):
        assert L.mpdata_plan_courant_device(p._p, sl0, n, ptr, None) == M.EINVAL, (sl0, n)
    assert L.mpdata_plan_courant_device(p._p, 0, ncrms, None, None) == M.EINVAL
    assert code(M, p.courant, 0, ncrms) == -1
    p.sync()
    assert not out.any()
    p.close()


def test_multi_gpu_handle_and_shard_plan(mpdata, oracle, monkeypatch):
    M = mpdata
    monkeypatch.delenv("MPDATA_MULTI_XFER", raising=False)
    name = "f64-blocks"
    shape, T, dt, _ = LM.INPUTS[name]
    ncrms, nx, nz = shape
    inp = CM.make(oracle, name)
    p = new_plan(M, name, devices=[0, 0])
    upload(p, inp)
    assert code(M, cour, p, dt, nz - 1, 0, ncrms) == M.EUNSUPPORTED
    assert b"mpdata_plan_shard_plan" in M.lib().mpdata_last_error()
    assert code(M, p.courant_host, 0, ncrms) == M.EUNSUPPORTED
    for g, (_, s0, nloc) in enumerate(p.shards()):
        q = p.shard_plan(g)
        same(cour(q, dt, nz - 1, 0, nloc), model(inp["u"], inp["w"], inp["rho"], inp["adz"], s0, nloc), f"shard {g}")
        q.close()
    p.close()
