"""GPU tests of the mass-weighted column integrals of a resident plan (include/mpdata_hip.h 3k):
mpdata_plan_column_path_device, the host forms, the array forms and their Python face Plan.column_path /
column_path_host / column_path.

Every comparison is bit for bit (util.assert_bitwise) against the numpy model of tests/column_path_model.py -- an explicit
loop over k in the array's dtype, the weight formed first, the product rounded before the add -- applied to a
reference-layout truth: the uploaded f, the CPU oracle's f after an EXACT run, else the plan's own whole export (existing
code; the feature under test is the reduction, not the advection), with the uploaded rho and adz.  Every output lies inside
a larger buffer with a patterned band of 4 KiB on both sides that must come back unchanged.

Shapes (tests/level_stats_model.py INPUTS): nz 3 .. 58 put 8, 4, 2 or 1 instances in a tile (nz 28: 27 levels per
instance, which straddle the 16-element lines of the chunk and its main / rest split), nz 72 and 130 are one-instance
tiles of two and three 64-element slices, 3 x 7 x 250 are five windows per instance with seams.  Those plans all fit ONE
workgroup group of the plan-layout kernel (16 adjacent 8-byte elements of the instance axis, 32 at nz <= 8); the plans of
CP.GROUP_INPUTS (section 7) need two or three, and their blocks start in the second group, straddle a group boundary and end
inside a group."""
import ctypes

import numpy as np
import pytest

import column_path_model as CP
import level_stats_model as LM
from plan_harness import BAND, _defaults, banded, tdt, upload
from test_plan_level_stats import BLOCKS, KINDS, new_plan, whole_export
from util import assert_bitwise, to_dev, to_host

pytestmark = pytest.mark.gpu


def bands_ok(bufs):
    import torch
    for k, (raw, orig, _) in bufs.items():
        assert torch.equal(raw[:BAND], orig[:BAND]) and torch.equal(raw[-BAND:], orig[-BAND:]), f"{k}: a band byte changed"


def paths(M, p, dt, nx, sl0, n, first=0, ntr=None, mass=True):
    """Plan.column_path into banded buffers -> (path (n, nx[, ntr]), mass (n[, ntr]) or None), Fortran order; the bands
    are checked"""
    import torch
    sh = M.column_path_shapes(n, nx, ntr)
    bufs = {k: banded(sh[k], dt) for k in (("path", "mass") if mass else ("path",))}
    torch.cuda.synchronize()      # (the plan may run on a stream that does not wait for the one that filled the buffers)
    p.column_path(bufs["path"][2], bufs["mass"][2] if mass else None, sl0, n, first)
    p.sync()
    bands_ok(bufs)
    return to_host(bufs["path"][2]), (to_host(bufs["mass"][2]) if mass else None)


def model(F, inp):
    assert np.all(np.isfinite(np.asarray(F)[:, 3:-3]))
    return CP.column_path(F, inp["rho"], inp["adz"])


def same(got, want, what):
    for k, g, w in zip(("path", "mass"), got, want):
        if g is None:
            continue
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape)
        assert_bitwise(g, w, f"{what}: {k}")


def check_whole(M, p, name, F, inp, what):
    shape, T, dt, _ = LM.INPUTS[name]
    same(paths(M, p, dt, shape[1], 0, shape[0], 0, None if T == 1 else T), model(F, inp), f"{name} {what}")


# ---- 1. every kind of plan, every state
@pytest.mark.parametrize("name,sw,note", KINDS, ids=[f"{k}{'-' + n if n else ''}" for k, _, n in KINDS])
def test_every_plan_kind_and_state(mpdata, oracle, name, sw, note):
    M = mpdata
    shape, T, dt, _ = LM.INPUTS[name]
    ncrms, nx, nz = shape
    inp = CP.make(oracle, name)
    p = new_plan(M, name, **sw)
    want_layout = M.LAYOUT_REFERENCE if (sw.get("ref") or "reference-layout" in note) else M.LAYOUT_WAVEMAJOR
    assert p.layout == want_layout and (p.level_windows > 1) == bool(sw.get("tall"))
    upload(p, inp)
    check_whole(M, p, name, inp["f"], inp, "after the upload")
    p.run()
    check_whole(M, p, name, oracle.advect(inp)[0], inp, "after one EXACT run")
    p.set_boundary(M.BOUNDARY_PERIODIC)
    p.run()
    p.run()
    got = paths(M, p, dt, nx, 0, ncrms, 0, None if T == 1 else T)       # while the halos are stale
    same(got, model(whole_export(M, p, name), inp), f"{name} after two periodic runs")
    p.set_boundary(M.BOUNDARY_GIVEN)
    other = CP.make(oracle, name, 50)
    p.run_uw(to_dev(other["u"]), to_dev(other["w"]))                   # the plan holds no velocities now
    check_whole(M, p, name, whole_export(M, p, name), inp, "after run_uw")
    p.import_block(ncrms - 1, f=to_dev(np.asfortranarray(other["f"][ncrms - 1:])))
    F = whole_export(M, p, name)
    assert_bitwise(F[ncrms - 1:], other["f"][ncrms - 1:], "the imported block")
    check_whole(M, p, name, F, inp, "after a block import of the last instance")
    p.close()
    p = new_plan(M, name, variant=M.VARIANT_FAST, **sw)
    upload(p, inp)
    check_whole(M, p, name, inp["f"], inp, "FAST after the upload")
    p.run()
    check_whole(M, p, name, whole_export(M, p, name), inp, "FAST after one run")
    p.close()


# ---- 2. blocks: odd starts and ends that split fp32 pairs, tiles and groups; a tracer sub-range
BLOCK_PLANS = [("f64-blocks", {}), ("f32-blocks", dict(odd=True)), ("f64-tall-blocks", dict(tall=True)),
               ("f32-tall-blocks", dict(tall=True, odd=True))]


@pytest.mark.parametrize("name,sw", BLOCK_PLANS, ids=lambda v: v if isinstance(v, str) else "")
def test_blocks_are_slices_of_the_whole(mpdata, oracle, name, sw):
    M = mpdata
    shape, T, dt, _ = LM.INPUTS[name]
    ncrms, nx, nz = shape
    assert ncrms == 11
    inp = CP.make(oracle, name)
    p = new_plan(M, name, **sw)
    assert p.layout == M.LAYOUT_WAVEMAJOR
    upload(p, inp)
    p.run()
    ntr = None if T == 1 else T
    W = paths(M, p, dt, nx, 0, ncrms, 0, ntr)
    same(W, model(oracle.advect(inp)[0], inp), f"{name} whole")
    for sl0, n in BLOCKS:
        got = paths(M, p, dt, nx, sl0, n, 0, ntr)
        same(got, tuple(np.asfortranarray(v[sl0:sl0 + n]) for v in W), f"{name} block {sl0, n}")
        if T == 3:
            got = paths(M, p, dt, nx, sl0, n, 1, 2)
            same(got, tuple(np.asfortranarray(v[sl0:sl0 + n, ..., 1:3]) for v in W), f"{name} block {sl0, n}, tracers 1..2")
    if T == 3:
        got = paths(M, p, dt, nx, 2, 7, 2, None)
        same(got, tuple(np.asfortranarray(v[2:9, ..., 2]) for v in W), f"{name} tracer 2 alone, a block")
        with pytest.raises(M.MpdataError) as e:
            paths(M, p, dt, nx, 0, ncrms, 2, 2)
        assert e.value.code == M.EINVAL
    p.close()


# ---- 3. mass skipped or given, device and host forms
@pytest.mark.parametrize("name,sw", BLOCK_PLANS + [("f32-nz12-ref", dict(ref=True)), ("f64-nz12-ref", dict(ref=True))],
                         ids=lambda v: v if isinstance(v, str) else "")
def test_mass_optional_and_host_forms(mpdata, oracle, name, sw):
    M = mpdata
    shape, T, dt, _ = LM.INPUTS[name]
    ncrms, nx, nz = shape
    inp = CP.make(oracle, name)
    p = new_plan(M, name, **sw)
    upload(p, inp)
    want = model(inp["f"], inp)
    ntr = None if T == 1 else T
    tail = (T,) if T > 1 else ()
    for sl0, n in ((0, ncrms), (1, ncrms - 2), (ncrms - 1, 1)):          # (the staging buffer grows and is reused)
        cut = tuple(np.asfortranarray(v[sl0:sl0 + n]) for v in want)
        dev = paths(M, p, dt, nx, sl0, n, 0, ntr)
        same(dev, cut, f"{name} device {sl0, n}")
        alone = paths(M, p, dt, nx, sl0, n, 0, ntr, mass=False)
        assert alone[1] is None
        same(alone, cut, f"{name} device, mass=None {sl0, n}")
        hp, hm = np.full((n, nx) + tail, -7, dt, order="F"), np.full((n,) + tail, -7, dt, order="F")
        p.column_path_host(hp, hm, sl0, n)
        same((hp, hm), dev, f"{name} host against device {sl0, n}")
        hp2 = np.full((n, nx) + tail, -7, dt, order="F")
        p.column_path_host(hp2, None, sl0, n)
        assert_bitwise(hp2, hp, f"{name} host, mass=None {sl0, n}")
    # the form of the other precision, and a null path
    other = np.float32 if dt == np.float64 else np.float64
    a = np.zeros((ncrms, nx) + tail, other, order="F")
    fn = M.lib().mpdata_plan_column_path_f32 if dt == np.float64 else M.lib().mpdata_plan_column_path
    assert fn(p._p, 0, ncrms, ctypes.c_void_p(a.ctypes.data), None) == M.ESTATE
    assert not a.any()
    mine = M.lib().mpdata_plan_column_path if dt == np.float64 else M.lib().mpdata_plan_column_path_f32
    assert mine(p._p, 0, ncrms, None, None) == M.EINVAL
    assert M.lib().mpdata_plan_column_path_device(p._p, 0, ncrms, None, None, 0, 1) == M.EINVAL
    p.close()


# ---- 4. the array forms, on a stream of their own
@pytest.mark.parametrize("name", ["f64-array", "f32-array"])
def test_array_forms(mpdata, oracle, name):
    import torch
    M = mpdata
    shape, T, dt, _ = LM.INPUTS[name]
    assert (shape, T) == ((7, 5, 6), 2)
    ncrms, nx, nz = shape
    inp = CP.make(oracle, name)
    want = model(inp["f"], inp)
    f, rho, adz = to_dev(inp["f"]), to_dev(inp["rho"]), to_dev(inp["adz"])
    keep = f.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    sh = M.column_path_shapes(ncrms, nx, T)
    bufs = {k: banded(sh[k], dt) for k in ("path", "mass")}
    M.column_path(f, rho, adz, bufs["path"][2], bufs["mass"][2], stream=s)
    s.synchronize()
    same((to_host(bufs["path"][2]), to_host(bufs["mass"][2])), want, name)
    bands_ok(bufs)
    assert torch.equal(f, keep)
    only = banded(sh["path"], dt)
    M.column_path(f, rho, adz, only[2])                    # the current stream, no mass
    torch.cuda.synchronize()
    assert_bitwise(to_host(only[2]), want[0], f"{name} path alone")
    bands_ok({"path": only})
    one = to_dev(np.asfortranarray(inp["f"][..., 1]))      # a 3-d f: one tracer, outputs without the tracer axis
    sh1 = M.column_path_shapes(ncrms, nx)
    o = {k: banded(sh1[k], dt) for k in ("path", "mass")}
    M.column_path(one, rho, adz, o["path"][2], o["mass"][2])
    torch.cuda.synchronize()
    same((to_host(o["path"][2]), to_host(o["mass"][2])), tuple(np.asfortranarray(v[..., 1]) for v in want), f"{name} one tracer")
    bands_ok(o)


# ---- 5. nothing of the plan changes
@pytest.mark.parametrize("name,sw,periodic", [("f64-blocks", {}, False), ("f64-tall-blocks", dict(tall=True), False),
                                              ("f32-blocks", dict(odd=True), True)], ids=lambda v: v if isinstance(v, str) else "")
def test_state_untouched(mpdata, oracle, name, sw, periodic):
    """a plan that makes the call between its runs against a twin that never does: export_device of f and flux,
    last_kernel_ms, and a following run"""
    import torch
    M = mpdata
    shape, T, dt, _ = LM.INPUTS[name]
    ncrms, nx, nz = shape
    inp = CP.make(oracle, name)
    ntr = None if T == 1 else T

    def export(p):
        sh = M.shapes(*shape, T)
        f = torch.empty(sh["f"], dtype=tdt(dt), device="cuda:0")
        fl = torch.empty(sh["flux"], dtype=tdt(dt), device="cuda:0")
        p.export_device(f=f, flux=fl)
        p.sync()
        return to_host(f), to_host(fl)

    def play(call):
        p = new_plan(M, name, **sw)
        if periodic:
            p.set_boundary(M.BOUNDARY_PERIODIC)
        upload(p, inp)
        p.run()
        p.sync()
        ms = p.last_kernel_ms()
        out = []
        if call:
            paths(M, p, dt, nx, 0, ncrms, 0, ntr)
            paths(M, p, dt, nx, 3, 5, 0, ntr, mass=False)
            hp = np.zeros((ncrms, nx) + ((T,) if T > 1 else ()), dt, order="F")
            p.column_path_host(hp)
            assert p.last_kernel_ms() == ms, "last_kernel_ms moved"
        out.append(export(p))
        p.run()
        if call:
            paths(M, p, dt, nx, 0, ncrms, 0, ntr)
        p.run()
        out.append(export(p))
        p.close()
        return out

    plain, called = play(False), play(True)
    for i, (a, b) in enumerate(zip(plain, called)):
        assert_bitwise(b[0], a[0], f"{name}: f of export {i} with and without the calls")
        assert_bitwise(b[1], a[1], f"{name}: flux of export {i} with and without the calls")


# ---- 6. errors on a live plan
def _code(M, fn, *a, **kw):
    with pytest.raises(M.MpdataError) as e:
        fn(*a, **kw)
    return e.value.code


def test_errors(mpdata, oracle):
    import torch
    M = mpdata
    name = "f64-blocks"
    shape, T, dt, _ = LM.INPUTS[name]
    ncrms, nx, nz = shape
    p = new_plan(M, name)
    raw, orig, out = banded((T, nx, ncrms), dt)
    rawm, origm, mass = banded((T, ncrms), dt)
    torch.cuda.synchronize()
    assert _code(M, p.column_path, out, mass) == M.ESTATE                     # never filled
    h = np.zeros((ncrms, nx, T), order="F")
    assert _code(M, p.column_path_host, h) == M.ESTATE
    upload(p, CP.make(oracle, name))
    ptr, pm = ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(mass.data_ptr())
    L = M.lib()
    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, ncrms + 1), (ncrms, 1), (5, 7)):
        assert L.mpdata_plan_column_path_device(p._p, sl0, n, ptr, pm, 0, 1) == M.EINVAL, (sl0, n)
    for first, cnt in ((-1, 1), (0, 0), (0, T + 1), (T, 1)):
        assert L.mpdata_plan_column_path_device(p._p, 0, ncrms, ptr, pm, first, cnt) == M.EINVAL, (first, cnt)
    assert L.mpdata_plan_column_path_device(p._p, 0, ncrms, None, pm, 0, 1) == M.EINVAL
    p.sync()
    torch.cuda.synchronize()
    assert torch.equal(raw, orig) and torch.equal(rawm, origm), "a refused call wrote to its outputs"
    assert not h.any()
    p.close()


def test_multi_gpu_handle_and_shard_plan(mpdata, oracle, monkeypatch):
    M = mpdata
    monkeypatch.delenv("MPDATA_MULTI_XFER", raising=False)
    name = "f64-blocks"
    shape, T, dt, _ = LM.INPUTS[name]
    ncrms, nx, nz = shape
    inp = CP.make(oracle, name)
    p = new_plan(M, name, devices=[0, 0])
    upload(p, inp)
    want = model(inp["f"], inp)
    assert _code(M, paths, M, p, dt, nx, 0, ncrms, 0, T) == M.EUNSUPPORTED
    assert b"mpdata_plan_shard_plan" in M.lib().mpdata_last_error()
    assert _code(M, p.column_path_host, np.zeros((ncrms, nx, T), order="F")) == M.EUNSUPPORTED
    for g, (_, s0, nloc) in enumerate(p.shards()):
        q = p.shard_plan(g)
        same(paths(M, q, dt, nx, 0, nloc, 0, T), tuple(np.asfortranarray(v[s0:s0 + nloc]) for v in want), f"shard {g}")
        same(paths(M, q, dt, nx, 1, 3, 0, T), tuple(np.asfortranarray(v[s0 + 1:s0 + 4]) for v in want), f"shard {g} block")
        q.close()
    p.close()


# ---- 7. more than one group of the plan-layout kernel: the whole plan, and blocks whose first group is not group 0,
# that straddle a group boundary, that end inside a group
GROUP_SW = {"f64-g40-nz28": {}, "f32-g41-nz28-odd": dict(odd=True), "f64-g70-nz5": {}, "f64-g20-nz72": {},
            "f64-g20-tall": dict(tall=True), "f32-g37-tall-odd": dict(tall=True, odd=True)}


@pytest.mark.parametrize("name", list(CP.GROUP_INPUTS))
def test_several_groups(mpdata, oracle, name):
    M = mpdata
    shape, T, dt, _ = CP.GROUP_INPUTS[name]
    ncrms, nx, nz = shape
    sw = GROUP_SW[name]
    inp = CP.make(oracle, name)
    M.set_tall_columns(int(bool(sw.get("tall"))))
    M.set_f32_odd_ncrms(int(bool(sw.get("odd"))))
    p = M.Plan(*shape, T, dtype=dt)
    assert p.layout == M.LAYOUT_WAVEMAJOR and (p.level_windows > 1) == bool(sw.get("tall"))
    upload(p, inp)
    ntr = None if T == 1 else T
    want = model(inp["f"], inp)
    same(paths(M, p, dt, nx, 0, ncrms, 0, ntr), want, f"{name} whole, after the upload")
    p.run()
    want = model(oracle.advect(inp)[0], inp)
    same(paths(M, p, dt, nx, 0, ncrms, 0, ntr), want, f"{name} whole, after one EXACT run")
    for sl0, n in CP.group_blocks(name):
        cut = tuple(np.asfortranarray(v[sl0:sl0 + n]) for v in want)
        same(paths(M, p, dt, nx, sl0, n, 0, ntr), cut, f"{name} block {sl0, n}")
        same(paths(M, p, dt, nx, sl0, n, 0, ntr, mass=False), cut, f"{name} block {sl0, n}, mass=None")
        if T > 1:
            same(paths(M, p, dt, nx, sl0, n, 1, None), tuple(np.asfortranarray(v[..., 1]) for v in cut), f"{name} block {sl0, n}, tracer 1")
        hp, hm = (np.full((n, nx) + ((T,) if T > 1 else ()), -7, dt, order="F"), np.full((n,) + ((T,) if T > 1 else ()), -7, dt, order="F"))
        p.column_path_host(hp, hm, sl0, n)
        same((hp, hm), cut, f"{name} block {sl0, n}, host form")
    p.close()
