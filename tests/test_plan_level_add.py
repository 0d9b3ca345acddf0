"""GPU tests of the per-level increments of a resident plan (include/mpdata_hip.h 3i): mpdata_plan_level_add_device, the
host forms, the array forms and their Python face Plan.level_add / level_add_host / level_add.

Every comparison is bit for bit (util.assert_bitwise) against the numpy model of tests/level_add_model.py -- d broadcast
over the column axis in f's dtype, np.maximum(0, .) for CLIP -- applied to a reference-layout truth: the uploaded f, the
plan model's arrays (tests/level_add_model.py PlanModelAdd: oracle/plan_model.py with the new call; an EXACT plan's f and
flux are bit-identical to it), or, for FAST plans, the plan's own whole export before the add.  The first d added to an
uploaded f is the one the guard of tests/test_level_add_cpu.py covers (no sum is zero); wherever a CLIP result is compared
that the guard does not cover, -0.0 is canonicalised on both sides (AM.canon).  d lies inside a larger buffer with a
patterned band of 4 KiB on both sides; the bands and d itself must come back unchanged.

The plan kinds, blocks and shapes are those of tests/test_plan_level_stats.py (LM.INPUTS)."""
import ctypes

import numpy as np
import pytest

import level_add_model as AM
import level_stats_model as LM
import plan_harness as H
from oracle import plan_model as PM
from plan_harness import BAND, _defaults, banded, upload
from test_plan_level_stats import BLOCKS, KINDS, _code, new_plan
from util import assert_bitwise, to_dev, to_host

pytestmark = pytest.mark.gpu
MODES = [(AM.ADD, "add"), (AM.CLIP, "clip")]


def dev_d(d):
    """host d (n, nzm[, ntr]) -> (raw, pristine copy, device view ([ntr,] nzm, n)) between two bands"""
    import torch
    raw, _, view = banded(d.T.shape, d.dtype)
    view.copy_(to_dev(d))
    torch.cuda.synchronize()
    return raw, raw.clone(), view


def add(p, d, sl0=0, n=None, mode=AM.ADD, first=0):
    """Plan.level_add of a banded d; afterwards the bands and d are as they were"""
    import torch
    raw, orig, view = dev_d(d)
    p.level_add(view, sl0, n, mode, first)
    p.sync()
    assert torch.equal(raw, orig), "a byte of d or of its bands changed"


def whole(M, p, name, what=("f", "flux")):
    return H.whole(M, p, LM.INPUTS[name], what)


def same_as_model(M, p, name, m, what, canon=False):
    got, want = whole(M, p, name), m.export_device()
    for k in ("f", "flux"):
        g, w = (AM.canon(got[k]), AM.canon(want[k])) if canon and k == "f" else (got[k], want[k])
        assert_bitwise(g, w, f"{name} {what}: {k}")


def model_of(oracle, name, inp):
    shape, T, dt, _ = LM.INPUTS[name]
    m = AM.PlanModelAdd(oracle, *shape, T, dt)
    assert m.upload(inp) is None
    return m


def d_like(name, k, sl0=0, n=None):
    """the k-th d of a test on LM.INPUTS[name] (k = 0: the guarded one), rows sl0 .. sl0+n of the whole plan's"""
    shape, T, dt, _ = LM.INPUTS[name]
    d = AM.make_d(shape, T, dt, AM.SEEDS[name] + k)
    return np.asfortranarray(d[sl0:sl0 + (shape[0] - sl0 if n is None else n)])


# ---- 1. every kind of plan, both modes
@pytest.mark.parametrize("mode,mname", MODES, ids=[m for _, m in MODES])
@pytest.mark.parametrize("name,sw,note", KINDS, ids=[f"{k}{'-' + n if n else ''}" for k, _, n in KINDS])
def test_every_plan_kind(mpdata, oracle, name, sw, note, mode, mname):
    M = mpdata
    shape, T, dt, seed = LM.INPUTS[name]
    ncrms, nx, nz = shape
    clip = mode == AM.CLIP
    inp = LM.make(oracle, shape, T, dt, seed)
    p = new_plan(M, name, **sw)
    want_layout = M.LAYOUT_REFERENCE if (sw.get("ref") or "reference-layout" in note) else M.LAYOUT_WAVEMAJOR
    assert p.layout == want_layout and (p.level_windows > 1) == bool(sw.get("tall"))
    upload(p, inp)
    m = model_of(oracle, name, inp)
    # (a) upload -> add -> whole export = the model of the uploaded f (guarded: no canonicalisation); flux unchanged
    d0 = d_like(name, 0)
    add(p, d0, mode=mode)
    assert m.level_add(d0, mode=mode) is None
    F1 = AM.level_add(inp["f"], d0, clip)
    got = whole(M, p, name)
    assert_bitwise(got["f"].reshape(F1.shape, order="F"), F1, f"{name} (a) upload, {mname}: f")
    assert_bitwise(got["flux"].reshape(inp["flux"].shape, order="F"), inp["flux"], f"{name} (a) upload, {mname}: flux")
    # (b) one EXACT run -> f AND flux = the oracle on the model's arrays (a window's non-owned levels left behind, or
    # u / w damaged, show here)
    p.run()
    f2, fl2 = oracle.advect(dict(inp, f=F1))
    got = whole(M, p, name)
    assert_bitwise(got["f"].reshape(f2.shape, order="F"), f2, f"{name} (b) add, run: f")
    assert_bitwise(got["flux"].reshape(fl2.shape, order="F")[:, :nz - 1], fl2[:, :nz - 1], f"{name} (b) add, run: flux")
    assert m.run() is None
    same_as_model(M, p, name, m, "(b) against the plan model")
    # (c) PERIODIC: run, add while the halos are stale, run
    p.set_boundary(M.BOUNDARY_PERIODIC)
    assert m.set_boundary(PM.PERIODIC) is None
    p.run()
    assert m.run() is None
    d1 = d_like(name, 1)
    add(p, d1, mode=mode)
    assert m.level_add(d1, mode=mode) is None
    p.run()
    assert m.run() is None
    same_as_model(M, p, name, m, f"(c) periodic: run, {mname}, run")
    # ... and once more while the halos are wrapped (the export above wrapped them)
    d2 = d_like(name, 2)
    add(p, d2, mode=mode)
    assert m.level_add(d2, mode=mode) is None
    same_as_model(M, p, name, m, f"(c) periodic: {mname} on wrapped halos", canon=clip)
    # (d) GIVEN: run_uw, add
    p.set_boundary(M.BOUNDARY_GIVEN)
    assert m.set_boundary(PM.GIVEN) is None
    other = LM.make(oracle, shape, T, dt, seed + 50)
    p.run_uw(to_dev(other["u"]), to_dev(other["w"]))
    assert m.run_uw(other["u"], other["w"]) is None
    d3 = d_like(name, 3)
    add(p, d3, mode=mode)
    assert m.level_add(d3, mode=mode) is None
    same_as_model(M, p, name, m, f"(d) run_uw, {mname}", canon=clip)
    p.close()
    # FAST: the same bits as EXACT on the uploaded f; after a run against the plan's own export changed by the model
    p = new_plan(M, name, variant=M.VARIANT_FAST, **sw)
    upload(p, inp)
    add(p, d0, mode=mode)
    assert_bitwise(whole(M, p, name, ("f",))["f"].reshape(F1.shape, order="F"), F1, f"{name} FAST upload, {mname}")
    p.run()
    E = whole(M, p, name, ("f",))["f"].reshape(F1.shape, order="F")
    add(p, d1, mode=mode)
    got = whole(M, p, name, ("f",))["f"].reshape(F1.shape, order="F")
    want = AM.level_add(E, d1, clip)
    assert_bitwise(AM.canon(got) if clip else got, AM.canon(want) if clip else want, f"{name} FAST run, {mname}")
    p.close()


# ---- 2. blocks: odd starts and ends that split fp32 pairs and tiles; CLIP, so that a touched neighbour shows
@pytest.mark.parametrize("name,sw", [("f64-blocks", {}), ("f32-blocks", dict(odd=True)), ("f64-tall-blocks", dict(tall=True)),
                                     ("f32-tall-blocks", dict(tall=True, odd=True))], ids=lambda v: v if isinstance(v, str) else "")
def test_blocks_leave_the_rest_alone(mpdata, oracle, name, sw):
    M = mpdata
    shape, T, dt, seed = LM.INPUTS[name]
    ncrms, nx, nz = shape
    assert ncrms == 11
    inp = LM.make(oracle, shape, T, dt, seed)
    p = new_plan(M, name, **sw)
    assert p.layout == M.LAYOUT_WAVEMAJOR
    upload(p, inp)
    for sl0, n in BLOCKS:
        # negative values and -0.0 in every instance OUTSIDE the block: a clip or a + 0.0 there changes bits
        F0 = np.array(inp["f"], order="F")
        out = np.ones(ncrms, bool)
        out[sl0:sl0 + n] = False
        flat = F0[out].reshape(-1)
        flat[0::3] = -flat[0::3]
        flat[1::7] = -0.0
        F0[out] = flat.reshape(F0[out].shape)
        assert n == ncrms or (LM.has_negative_zero(F0[out]) and np.any(F0[out] < 0))
        p.import_device(f=to_dev(F0))
        d = d_like(name, 0, sl0, n)
        add(p, d, sl0, n, AM.CLIP)
        got = whole(M, p, name, ("f",))["f"].reshape(F0.shape, order="F")
        assert_bitwise(got[out], F0[out], f"{name} block {sl0, n}: outside")
        assert_bitwise(got[sl0:sl0 + n], AM.level_add(inp["f"][sl0:sl0 + n], d, True), f"{name} block {sl0, n}: inside")
        if (sl0, n) == (10, 1) and sw.get("odd"):
            # the phantom half followed instance ncrms - 1: a run of that instance matches the oracle
            Fm = np.array(F0, order="F")
            Fm[10:] = AM.level_add(inp["f"][10:], d, True)
            f2, fl2 = oracle.advect(dict(inp, f=Fm))
            p.run()
            got = whole(M, p, name)
            assert_bitwise(got["f"].reshape(f2.shape, order="F")[10:], f2[10:], f"{name} block (10, 1), run: f of instance 10")
            assert_bitwise(got["flux"].reshape(fl2.shape, order="F")[10:, :nz - 1], fl2[10:, :nz - 1],
                           f"{name} block (10, 1), run: flux of instance 10")
            p.import_device(flux=to_dev(inp["flux"]))
    p.close()


# ---- 3. tracer ranges: d holds only the range's tracers, the others keep their bits
@pytest.mark.parametrize("name,sw", [("f64-blocks", {}), ("f32-blocks", dict(odd=True)), ("f64-nz12-ref", dict(ref=True))],
                         ids=lambda v: v if isinstance(v, str) else "")
def test_tracer_ranges(mpdata, oracle, name, sw):
    M = mpdata
    shape, T, dt, seed = LM.INPUTS[name]
    ncrms, nx, nz = shape
    assert T == 3
    inp = LM.make(oracle, shape, T, dt, seed)
    p = new_plan(M, name, **sw)
    upload(p, inp)
    m = model_of(oracle, name, inp)
    d = d_like(name, 0)
    for mode, sl0, n, first, dd in ((AM.CLIP, 0, ncrms, 1, np.asfortranarray(d[..., 1:3])),          # tracers 1..2, 3-d d
                                    (AM.ADD, 2, 7, 2, np.asfortranarray(d[2:9, :, 2])),               # tracer 2, a block, 2-d d
                                    (AM.ADD, 0, ncrms, 0, np.asfortranarray(d[..., 0:1]))):           # tracer 0, 3-d d of one
        before = whole(M, p, name, ("f",))["f"]
        add(p, dd, sl0, n, mode, first)
        assert m.level_add(dd, sl0, n, mode, first) is None
        ntr = dd.shape[2] if dd.ndim == 3 else 1
        got = whole(M, p, name, ("f",))["f"]
        rest = [t for t in range(T) if not first <= t < first + ntr]
        assert_bitwise(got[..., rest], before[..., rest], f"{name} tracers {first}..{first + ntr - 1}: the other tracers")
        assert_bitwise(AM.canon(got), AM.canon(m.a["f"]), f"{name} tracers {first}..{first + ntr - 1}")
    raw, orig, view = dev_d(np.asfortranarray(d[..., 0:2]))
    assert _code(M, p.level_add, view, 0, ncrms, AM.ADD, 2) == M.EINVAL        # two tracers from tracer 2
    p.close()


# ---- 4. two adds in a row are two roundings
@pytest.mark.parametrize("name,sw", [("f64-blocks", {}), ("f32-blocks", dict(odd=True)), ("f64-nz12-ref", dict(ref=True)),
                                     ("f64-tall", dict(tall=True))], ids=lambda v: v if isinstance(v, str) else "")
def test_two_adds_in_a_row(mpdata, oracle, name, sw):
    M = mpdata
    shape, T, dt, seed = LM.INPUTS[name]
    inp = LM.make(oracle, shape, T, dt, seed)
    p = new_plan(M, name, **sw)
    upload(p, inp)
    d0, d1 = d_like(name, 0), d_like(name, 1)
    add(p, d0)
    add(p, d1)
    two = AM.level_add(AM.level_add(inp["f"], d0), d1)
    assert np.any(LM.bits(two) != LM.bits(AM.level_add(inp["f"], d0 + d1)))
    assert_bitwise(whole(M, p, name, ("f",))["f"].reshape(two.shape, order="F"), two, f"{name}: two adds")
    p.close()


# ---- 5. the array forms: f between bands, both modes, a stream of their own
@pytest.mark.parametrize("mode,mname", MODES, ids=[m for _, m in MODES])
@pytest.mark.parametrize("name", ["f64-array", "f32-array"])
def test_array_forms(mpdata, oracle, name, mode, mname):
    import torch
    M = mpdata
    shape, T, dt, seed = LM.INPUTS[name]
    assert (shape, T) == ((7, 5, 6), 2)
    F = LM.make(oracle, shape, T, dt, seed)["f"]
    d = d_like(name, 0)
    want = AM.level_add(F, d, mode == AM.CLIP)
    fraw, forig, fview = banded(F.T.shape, dt)
    fview.copy_(to_dev(F))
    draw, dorig, dview = dev_d(d)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    M.level_add(fview, dview, mode, stream=s)
    s.synchronize()
    assert_bitwise(to_host(fview), want, f"{name} {mname}")
    assert torch.equal(fraw[:BAND], forig[:BAND]) and torch.equal(fraw[-BAND:], forig[-BAND:]), "a band byte of f changed"
    assert torch.equal(draw, dorig), "a byte of d or of its bands changed"
    one = to_dev(np.asfortranarray(F[..., 1]))                  # a 3-d f: one tracer, a 2-d d; the current stream
    M.level_add(one, to_dev(np.asfortranarray(d[..., 1])), mode)
    torch.cuda.synchronize()
    assert_bitwise(to_host(one), np.asfortranarray(want[..., 1]), f"{name} {mname} one tracer")
    assert _code(M, M.level_add, one, to_dev(np.asfortranarray(d[..., 1])), 2) == M.EINVAL
    assert_bitwise(to_host(one), np.asfortranarray(want[..., 1]), f"{name}: f after an unknown mode")


# ---- 6. the host forms
@pytest.mark.parametrize("name,sw", [("f64-blocks", {}), ("f32-blocks", dict(odd=True)), ("f32-nz12-ref", dict(ref=True)),
                                     ("f64-tall", dict(tall=True))], ids=lambda v: v if isinstance(v, str) else "")
def test_host_forms(mpdata, oracle, name, sw):
    M = mpdata
    shape, T, dt, seed = LM.INPUTS[name]
    ncrms, nx, nz = shape
    inp = LM.make(oracle, shape, T, dt, seed)
    p = new_plan(M, name, **sw)
    upload(p, inp)
    m = model_of(oracle, name, inp)
    for k, (sl0, n, mode) in enumerate(((ncrms - 1, 1, AM.ADD), (1, ncrms - 2, AM.CLIP), (0, ncrms, AM.ADD))):   # (the staging buffer grows)
        d = d_like(name, k, sl0, n)
        keep = d.copy(order="F")
        p.level_add_host(d, sl0, n, mode)
        assert_bitwise(d, keep, "the caller's d")
        assert m.level_add(d, sl0, n, mode) is None
        same_as_model(M, p, name, m, f"host form {sl0, n}", canon=True)
    # the form of the other precision
    before = whole(M, p, name)
    other = np.float32 if dt == np.float64 else np.float64
    a = np.ones((ncrms, nz - 1) + ((T,) if T > 1 else ()), other, order="F")
    fn = M.lib().mpdata_plan_level_add_f32 if dt == np.float64 else M.lib().mpdata_plan_level_add
    assert fn(p._p, 0, ncrms, ctypes.c_void_p(a.ctypes.data), AM.ADD) == M.ESTATE
    assert M.lib().mpdata_plan_level_add(p._p, 0, ncrms, None, AM.ADD) == M.EINVAL
    after = whole(M, p, name)
    for k in before:
        assert_bitwise(after[k], before[k], f"{name}: {k} after refused host calls")
    p.close()


# ---- 7. errors: the code, and the whole export bit-identical afterwards
def test_errors(mpdata, oracle):
    import torch
    M = mpdata
    name = "f64-blocks"
    shape, T, dt, seed = LM.INPUTS[name]
    ncrms, nx, nz = shape
    inp = LM.make(oracle, shape, T, dt, seed)
    d = d_like(name, 0)
    dev = to_dev(d)
    p = new_plan(M, name)
    m = AM.PlanModelAdd(oracle, *shape, T, dt)
    assert _code(M, p.level_add, dev) == M.ESTATE == m.level_add(d)                         # never filled
    assert _code(M, p.level_add_host, d) == M.ESTATE
    upload(p, inp)
    assert m.upload(inp) is None
    before = whole(M, p, name)
    L = M.lib()
    ptr = ctypes.c_void_p(dev.data_ptr())
    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, ncrms + 1), (ncrms, 1), (5, 7)):
        assert L.mpdata_plan_level_add_device(p._p, sl0, n, ptr, AM.ADD, 0, 1) == M.EINVAL == m.level_add(d[..., 0], sl0, n), (sl0, n)
        assert L.mpdata_plan_level_add(p._p, sl0, n, ctypes.c_void_p(d.ctypes.data), AM.ADD) == M.EINVAL, (sl0, n)
    for first, cnt in ((-1, 1), (0, 0), (0, T + 1), (T, 1), (2, 2)):
        assert L.mpdata_plan_level_add_device(p._p, 0, ncrms, ptr, AM.ADD, first, cnt) == M.EINVAL, (first, cnt)
    assert m.level_add(d, first=1) == M.EINVAL and m.level_add(d[..., 0], first=T) == M.EINVAL
    for mode in (-1, 2, 7):
        assert L.mpdata_plan_level_add_device(p._p, 0, ncrms, ptr, mode, 0, T) == M.EINVAL == m.level_add(d, mode=mode), mode
        assert L.mpdata_plan_level_add(p._p, 0, ncrms, ctypes.c_void_p(d.ctypes.data), mode) == M.EINVAL
    assert b"unknown mode" in L.mpdata_last_error()
    assert L.mpdata_plan_level_add_device(p._p, 0, ncrms, None, AM.ADD, 0, T) == M.EINVAL == m.level_add(None)
    assert L.mpdata_plan_level_add_device(None, 0, ncrms, ptr, AM.ADD, 0, T) == M.EINVAL
    assert L.mpdata_plan_level_add_f32(p._p, 0, ncrms, ctypes.c_void_p(d.ctypes.data), AM.ADD) == M.ESTATE
    p.sync()
    after = whole(M, p, name)
    for k in before:
        assert_bitwise(after[k], before[k], f"{k} after the refused calls")
        assert_bitwise(after[k], m.a[k], f"{k} against the model")
    assert torch.equal(dev, to_dev(d))
    p.close()


def test_multi_gpu_handle_and_shard_plan(mpdata, oracle, monkeypatch):
    M = mpdata
    monkeypatch.delenv("MPDATA_MULTI_XFER", raising=False)
    name = "f64-blocks"
    shape, T, dt, seed = LM.INPUTS[name]
    ncrms, nx, nz = shape
    inp = LM.make(oracle, shape, T, dt, seed)
    d = d_like(name, 0)
    p = new_plan(M, name, devices=[0, 0])
    upload(p, inp)
    m = model_of(oracle, name, inp)
    m.multi = True
    assert _code(M, p.level_add, to_dev(d)) == M.EUNSUPPORTED == m.level_add(d)
    assert b"mpdata_plan_shard_plan" in M.lib().mpdata_last_error()
    assert _code(M, p.level_add_host, d) == M.EUNSUPPORTED
    m.multi = False
    same_as_model(M, p, name, m, "after the refused handle calls")
    for g, (_, s0, nloc) in enumerate(p.shards()):
        q = p.shard_plan(g)
        dd = np.asfortranarray(d[s0:s0 + nloc])
        add(q, dd, mode=AM.CLIP)
        assert m.level_add(dd, s0, nloc, AM.CLIP) is None
        blk = np.asfortranarray(d_like(name, 1)[s0 + 1:s0 + 4, :, 1])
        add(q, blk, 1, 3, AM.ADD, 1)
        assert m.level_add(blk, s0 + 1, 3, AM.ADD, 1) is None
        q.close()
    same_as_model(M, p, name, m, "after the shard plans' adds", canon=True)
    p.run()
    assert m.run() is None
    same_as_model(M, p, name, m, "after the shard plans' adds and a run")
    p.close()


# ---- 8. no state change
@pytest.mark.parametrize("name,sw", [("f64-blocks", {}), ("f32-tall-blocks", dict(tall=True, odd=True))],
                         ids=lambda v: v if isinstance(v, str) else "")
def test_no_state_change(mpdata, oracle, name, sw):
    M = mpdata
    shape, T, dt, seed = LM.INPUTS[name]
    ncrms, nx, nz = shape
    inp = LM.make(oracle, shape, T, dt, seed)
    p = new_plan(M, name, **sw)
    upload(p, inp)
    assert _code(M, p.last_kernel_ms) == M.ESTATE           # no run yet
    add(p, d_like(name, 0))
    assert _code(M, p.last_kernel_ms) == M.ESTATE           # ... and the add is none
    p.run()
    p.sync()
    ms = p.last_kernel_ms()
    c0 = p.courant_host()
    add(p, d_like(name, 1), mode=AM.CLIP)
    add(p, d_like(name, 2, 3, 5), 3, 5)
    assert p.last_kernel_ms() == ms
    c1 = p.courant_host()
    assert_bitwise(c1[0], c0[0], "clev before and after")
    assert_bitwise(c1[1], c0[1], "cinst before and after")
    assert p.boundary == M.BOUNDARY_GIVEN
    p.set_timing(0)
    add(p, d_like(name, 3))
    assert _code(M, p.last_kernel_ms) == M.ESTATE           # the timing pair stays off
    p.set_timing(1)
    other = LM.make(oracle, shape, T, dt, seed + 50)
    p.run_uw(to_dev(other["u"]), to_dev(other["w"]))
    add(p, d_like(name, 4))
    assert _code(M, p.run) == M.ESTATE                       # still no velocities
    assert _code(M, p.courant_host) == M.ESTATE
    p.set_boundary(M.BOUNDARY_PERIODIC)
    add(p, d_like(name, 5))
    assert p.boundary == M.BOUNDARY_PERIODIC
    p.close()
