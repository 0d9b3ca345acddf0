"""GPU tests of the implicit vertical solve of a resident plan (include/mpdata_hip.h 3o): mpdata_plan_vsolve_device, the
host forms, the array forms, their Python face Plan.vsolve / vsolve_host / vsolve, and the Fortran program
tests/fortran/vsolve_calls.F90.

Every comparison is bit for bit (util.assert_bitwise) against the numpy model of tests/vsolve_model.py: VM.vsolve on a
reference-layout truth, or the plan model with the new call (VM.PlanModelVsolve: an EXACT plan's f and flux are
bit-identical to it), or, for FAST plans, the plan's own whole export before the call.  The whole export of f AND flux is
compared.  lo, di, up lie inside larger buffers with 4 KiB of NaN on both sides, so a read outside the block's arrays
poisons the result, and must come back unchanged.  lo, up are uniform in [-0.4, 0), di = 1 - lo - up; f is the oracle's
raw field moved by one half, so signed.  u and w have no export: that they keep their bits shows in the run behind the
calls, which is compared with the model's.

G = 16 is the group of the kernel: the adjacent 8-byte elements of the instance axis a workgroup owns (4 at 237 levels).
CB = 8 is the column batch of the kernel as built at 27 levels ((5120 / (16 * 27)) - 3), so nx = 11 is two batches of 6 and
5; at 237 levels a batch is 2 columns.  Shapes (ncrms, nx, nz): 37 instances are two full groups and a partial one, 5 less
than one; nx = 1 and 11; 1 and 3 tracers; nz = 2 (one level: the array forms only, a plan has 3 or more), 3, 28 (two slots per tile), 34 (one slot), 65 (a full wave),
66 (two slices), 72 (a tail wave), 130 (three slices), 238.  fp32: pairs (even, 37 pairs), the phantom (odd with the
switch, 19 elements), the reference layout (odd without it).  Windowed plans (nz > 238 with set_tall_columns): 239 and 300
levels fp64, 250 fp32, three groups of 239 levels, fp32 with an odd number of instances (an inner phantom)."""
import numpy as np
import pytest

import fortran_records as FR
import plan_harness as H
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
    "f64-nz34": ((5, 11, 34), 1, F64, {}), "f64-nz65": ((5, 1, 65), 1, F64, {}), "f64-nz66": ((5, 11, 66), 1, F64, {}),
    "f64-nz72": ((5, 3, 72), 3, F64, {}), "f64-nz130": ((5, 1, 130), 1, F64, {}), "f64-nz238": ((5, 11, 238), 1, F64, {}),
    "f32-nz28-even": ((6, 11, 28), 3, F32, {}), "f32-nz28-3groups": ((4 * G + 10, 1, 28), 1, F32, {}),
    "f32-nz72-even": ((6, 3, 72), 1, F32, {}),
    "f32-nz28-odd": ((2 * G + 5, 11, 28), 3, F32, dict(odd=True)), "f32-nz72-odd": ((5, 1, 72), 1, F32, dict(odd=True)),
    "f32-nz3-odd": ((5, 3, 3), 1, F32, dict(odd=True)),
    "f64-nz12-ref": ((5, 3, 12), 3, F64, dict(ref=True)),
    "f32-nz28-odd-ref": ((5, 3, 28), 1, F32, {}),      # (an odd fp32 plan without the switch keeps the reference layout)
    "f64-nz239-tall": ((5, 3, 239), 3, F64, dict(tall=True)), "f64-nz300-tall": ((5, 1, 300), 1, F64, dict(tall=True)),
    "f64-nz239-tall-3groups": ((2 * G + 5, 1, 239), 1, F64, dict(tall=True)),
    "f32-nz250-tall": ((6, 3, 250), 1, F32, dict(tall=True)),
    "f32-nz239-tall-odd": ((5, 2, 239), 3, F32, dict(tall=True, odd=True)),
}
REF = ("f64-nz12-ref", "f32-nz28-odd-ref")
# one kind of each family runs the FAST variant too; one of each a PERIODIC plan
FAST = ("f64-nz28-3groups", "f64-nz72", "f32-nz28-odd", "f64-nz12-ref", "f64-nz239-tall")
PERIODIC = ("f64-nz34", "f32-nz72-odd", "f64-nz12-ref", "f32-nz239-tall-odd", "f64-nz300-tall")
SEED = 100


_INPUTS = {}


def inputs(oracle, name):
    """the seven arrays of KINDS[name]: computed once and shared; no test writes them"""
    if name not in _INPUTS:
        shape, T, dt, _ = KINDS[name]
        _INPUTS[name] = VM.make_plan_inputs(oracle, shape, T, dt, SEED)
    return _INPUTS[name]


def new_plan(M, name, variant=None):
    return H.new_plan(M, KINDS[name], name, name in REF, bool(KINDS[name][3].get("tall")), variant)


def model_of(oracle, name):
    shape, T, dt, _ = KINDS[name]
    m = VM.PlanModelVsolve(oracle, *shape, T, dt)
    assert m.upload({k: np.array(v, order="F") for k, v in inputs(oracle, name).items()}) is None
    return m


def whole(M, p, name, what=("f", "flux")):
    return H.whole(M, p, KINDS[name], what)


def same_as_model(M, p, name, m, what):
    H.same_as_model(M, p, KINDS[name], name, m, what)


def coeffs_of(name, k, n=None):
    """(lo, di, up) (n, nzm) of a block, other values per k"""
    shape, T, dt, _ = KINDS[name]
    return VM.make_coeffs(shape[0] if n is None else n, shape[2], dt, 500 + k)


def vsolve(M, p, name, c, sl0=0, n=None, first=0, ntr=None, call=None):
    """Plan.vsolve of host lo, di, up (n, nzm) between NaN bands, which are checked unchanged.  call: another callable with
    Plan.vsolve's arguments (a shard plan's)."""
    import torch
    shape, T, dt, _ = KINDS[name]
    nz = shape[2]
    n = shape[0] - sl0 if n is None else n
    ntr = T - first if ntr is None else ntr
    sh = M.vsolve_shapes(n, nz)
    bufs = []
    for a, k in zip(c, ("lo", "di", "up")):
        assert a.shape == (n, nz - 1) and a.dtype == dt
        raw, view = nan_banded(a, sh[k])
        bufs.append((raw, raw.clone(), view))
    torch.cuda.synchronize()      # (the plan may run on a stream that does not wait for the one that filled the buffers)
    (call or p.vsolve)(bufs[0][2], bufs[1][2], bufs[2][2], sl0, n, first, ntr)
    p.sync()
    torch.cuda.synchronize()
    for (raw, orig, _), k in zip(bufs, ("lo", "di", "up")):
        assert torch.equal(raw.view(torch.uint8), orig.view(torch.uint8)), f"{k} changed"


# ---- 1. every kind of plan: upload -> vsolve -> compare -> run -> compare -> vsolve twice -> compare (-> run -> compare)
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
    # (a) upload -> vsolve -> the model on the uploaded f
    c0 = coeffs_of(name, 0)
    assert (F0 < 0).any() and (F0 > 0).any()
    vsolve(M, p, name, c0)
    want_f = VM.vsolve(F0, *c0)
    assert_bitwise(want_f[:, :3], F0[:, :3], "the halos stay")
    assert_bitwise(want_f[:, nx + 3:], F0[:, nx + 3:], "the halos stay")
    assert not np.array_equal(want_f, F0)
    assert m.vsolve(*c0) is None
    e = whole(M, p, name)
    assert_bitwise(e["f"], want_f, f"{name} (a): f")
    assert_bitwise(e["flux"], inp["flux"].reshape(e["flux"].shape, order="F"), f"{name} (a): flux")
    same_as_model(M, p, name, m, "(a) the plan model")
    # (b) a run on the kept velocities = export -> model -> import -> run: seams and the phantom are consistent
    p.run()
    assert m.run() is None
    same_as_model(M, p, name, m, "(b) vsolve, run")
    # (c) behind the run (a windowed plan's seams are stale), twice in a row (the second behind marks the first cleared)
    for k in (1, 2):
        c = coeffs_of(name, k)
        vsolve(M, p, name, c)
        assert m.vsolve(*c) is None
    same_as_model(M, p, name, m, "(c) run, vsolve, vsolve")
    p.run()
    assert m.run() is None
    same_as_model(M, p, name, m, "(c) run, vsolve, vsolve, run")
    if name in PERIODIC:
        # (d) PERIODIC: run, vsolve while the halos are stale; the export hands out wrapped halos of the NEW field
        p.set_boundary(M.BOUNDARY_PERIODIC)
        assert m.set_boundary(PM.PERIODIC) is None
        p.run()
        assert m.run() is None
        c = coeffs_of(name, 5)
        vsolve(M, p, name, c)
        assert m.vsolve(*c) is None
        same_as_model(M, p, name, m, "(d) periodic: run, vsolve")
        # ... on halos the export just wrapped: they are copies of the OLD field now, the next export wraps again
        c = coeffs_of(name, 6)
        vsolve(M, p, name, c)
        assert m.vsolve(*c) is None
        e = whole(M, p, name, ("f",))["f"]
        assert_bitwise(e, PM.wrap(np.array(e, order="F")), f"{name} (d): the halos are wrapped copies of the new interior")
        same_as_model(M, p, name, m, "(d) periodic: vsolve on wrapped halos")
        c = coeffs_of(name, 7)
        vsolve(M, p, name, c)
        assert m.vsolve(*c) is None
        p.run()
        assert m.run() is None
        same_as_model(M, p, name, m, "(d) periodic: vsolve, run")
        # ... and back to GIVEN behind a call: the plan holds what an export just before the switch would have returned
        c = coeffs_of(name, 8)
        vsolve(M, p, name, c)
        assert m.vsolve(*c) is None
        p.set_boundary(M.BOUNDARY_GIVEN)
        assert m.set_boundary(PM.GIVEN) is None
        same_as_model(M, p, name, m, "(d) periodic: vsolve, set_boundary(GIVEN)")
    p.close()
    if name in FAST:
        # FAST: the same bits as EXACT on the uploaded f; after a run against the plan's own export changed by the model
        p = new_plan(M, name, variant=M.VARIANT_FAST)
        upload(p, inp)
        vsolve(M, p, name, c0)
        assert_bitwise(whole(M, p, name, ("f",))["f"], want_f, f"{name} FAST upload, vsolve")
        p.run()
        E = whole(M, p, name, ("f",))["f"]
        c1 = coeffs_of(name, 1)
        vsolve(M, p, name, c1)
        assert_bitwise(whole(M, p, name, ("f",))["f"], VM.vsolve(E, *c1), f"{name} FAST run, vsolve")
        p.close()


# ---- 2. blocks and tracer sub-ranges: what lies outside keeps every bit
BLOCKS = {
    # two per tile, five instances: inside one group, one instance, the last one
    "f64-nz28": [(1, 3), (2, 1), (4, 1), (0, 5)],
    # three groups: a block that straddles a group boundary, odd sl0 across two boundaries, the last instance alone, a group
    "f64-nz28-3groups": [(G - 1, 3), (3, 2 * G), (2 * G + 4, 1), (G, G)],
    "f64-nz72": [(1, 1), (1, 2)],
    "f64-nz130": [(1, 1), (0, 1)],
    # fp32 pairs: odd sl0 and odd n (split pairs at both ends), one half, a whole pair
    "f32-nz28-even": [(1, 3), (5, 1), (2, 2)],
    # 37 pairs: across a group boundary (2G instances per group), splitting pairs
    "f32-nz28-3groups": [(2 * G - 1, 3), (1, 4 * G + 4), (4 * G + 9, 1)],
    # fp32 pairs, odd plan of 37 (instance 36 shares its pair with the phantom): blocks that hold and miss instance 36
    "f32-nz28-odd": [(1, 2), (36, 1), (35, 2), (0, 36), (33, 3), (0, 37)],
    "f32-nz72-odd": [(4, 1), (1, 1), (0, 2), (3, 2)],
    "f32-nz28-odd-ref": [(1, 3), (4, 1)],
    "f64-nz12-ref": [(1, 3), (4, 1)],
    # windowed plans: each behind an import (the first) and behind a run (the others: stale seams), a block and the whole
    "f64-nz239-tall": [(1, 1), (0, 1), (0, 2), (2, 3)],
    "f64-nz239-tall-3groups": [(G - 1, 3), (2 * G + 4, 1), (1, 2 * G)],
    "f32-nz239-tall-odd": [(1, 1), (4, 1), (0, 2), (3, 2), (0, 5)],
    "f32-nz250-tall": [(1, 3), (5, 1)],
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
        vsolve(M, p, name, c, sl0, n, first, ntr)
        assert m.vsolve(*c, sl0=sl0, n=n, first=first, ntr=ntr) is None
        after = whole(M, p, name)
        out = np.ones(ncrms, bool)
        out[sl0:sl0 + n] = False
        tout = np.ones(T, bool)
        tout[first:first + ntr] = False
        assert_bitwise(after["f"][out], before["f"][out], f"{name} block {sl0, n}: instances outside")
        assert_bitwise(after["f"][..., tout], before["f"][..., tout], f"{name} block {sl0, n}: tracers outside")
        assert_bitwise(after["flux"], before["flux"], f"{name} block {sl0, n}: flux")
        want = VM.vsolve(before["f"][sl0:sl0 + n, ..., first:first + ntr], *c)
        assert_bitwise(after["f"][sl0:sl0 + n, ..., first:first + ntr], want, f"{name} block {sl0, n}: inside")
        assert not np.array_equal(want, before["f"][sl0:sl0 + n, ..., first:first + ntr])
        # a run of every instance (the phantom of an odd plan rides with instance ncrms - 1; a windowed plan refreshes
        # the seams the call marked stale; u, w, rho, rhow, adz enter it) matches the model
        p.run()
        assert m.run() is None
        same_as_model(M, p, name, m, f"block {sl0, n}, run")
    p.close()


# ---- 3. the host forms equal the device form (both equal the model bit for bit)
@pytest.mark.parametrize("name", ["f64-nz28-3groups", "f32-nz28-odd", "f64-nz12-ref", "f64-nz72", "f64-nz239-tall", "f32-nz250-tall"])
def test_host_form(mpdata, oracle, name):
    M = mpdata
    shape, T, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    p = new_plan(M, name)
    upload(p, inputs(oracle, name))
    m = model_of(oracle, name)
    for k, (sl0, n) in enumerate(((0, ncrms), (1, 1), (ncrms - 1, 1), (0, 2))):
        c = coeffs_of(name, 20 + k, n)
        keep = [np.array(a, order="F") for a in c]
        p.vsolve_host(*c, sl0, n)
        for a, b, nm in zip(c, keep, ("lo", "di", "up")):
            assert_bitwise(a, b, f"{name} host {sl0, n}: {nm}")
        assert m.vsolve(*c, sl0=sl0, n=n) is None
        same_as_model(M, p, name, m, f"host form {sl0, n}")
        p.run()
        assert m.run() is None
        same_as_model(M, p, name, m, f"host form {sl0, n}, run")
    with pytest.raises(M.MpdataError):
        p.vsolve_host(c[0][:, :-1], c[1], c[2], sl0=0, n=2)       # a wrong shape
    p.close()


# 257 and 600 instances: more than one block of 256 threads and a partly filled last one; (2, 1, 3) with 32769 tracers:
# 65538 rows, the second trip over gridDim.y.  f is random, so instance b differs from b - 256 and row r from r - 65535.
# Each with a block inside the arrays; f lies between NaN bands that must come back unchanged.
# (5, 1, 2): one level, which no plan can have (mpdata_plan_create needs nz >= 3): x = f * (1 / di).
ARRAYS = {"nz2": ((5, 1, 2), 1, (1, 3)), "n257": ((257, 3, 6), 2, (1, 256)), "n600": ((600, 2, 5), 1, (300, 299)), "rows65538": ((2, 1, 3), 32769, (1, 1))}


@pytest.mark.parametrize("case", list(ARRAYS))
@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
def test_array_forms(mpdata, dt, case):
    import torch
    M = mpdata
    (ncrms, nx, nz), T, (b0, bn) = ARRAYS[case]
    rng = np.random.default_rng([77, ncrms, T])
    f = np.asfortranarray(rng.uniform(-1.0, 1.0, (ncrms, nx + 6, nz - 1, T)).astype(dt))
    for sl0, n in ((0, ncrms), (b0, bn)):
        c = VM.make_coeffs(n, nz, dt, 600 + sl0)
        full = np.array(f, order="F")
        full[sl0:sl0 + n] = VM.vsolve(f[sl0:sl0 + n], *c)
        if n > 256:
            assert not np.array_equal(full[sl0 + 256:sl0 + n], full[sl0:sl0 + n - 256])
        fraw, fd = nan_banded(f, (T, nz - 1, nx + 6, ncrms))
        pad = (fraw.numel() - fd.numel()) // 2
        sh = M.vsolve_shapes(n, nz)
        bufs = [nan_banded(a, sh[k]) for a, k in zip(c, ("lo", "di", "up"))]
        orig = [raw.clone() for raw, _ in bufs]
        torch.cuda.synchronize()
        M.vsolve(fd, bufs[0][1], bufs[1][1], bufs[2][1], sl0, n)
        torch.cuda.synchronize()
        assert torch.isnan(fraw[:pad]).all() and torch.isnan(fraw[-pad:]).all(), "a guard band of f changed"
        for (raw, _), o in zip(bufs, orig):
            assert torch.equal(raw.view(torch.uint8), o.view(torch.uint8)), "a coefficient array changed"
        assert_bitwise(to_host(fd), full, f"array form {case} block {sl0, n}: f")
    if T == 1 or case == "n257":
        # one tracer without the tracer axis
        f1 = to_dev(np.asfortranarray(f[..., 0]))
        c = VM.make_coeffs(ncrms, nz, dt, 650)
        M.vsolve(f1, *(to_dev(a) for a in c))
        torch.cuda.synchronize()
        assert_bitwise(to_host(f1), VM.vsolve(f[..., 0], *c), f"array form {case}, one tracer: f")


# ---- 4. every error code, in the stated order; the plan's state before and after
def test_errors_change_nothing(mpdata, oracle):
    M = mpdata
    name = "f64-nz72"
    shape, T, dt, _ = KINDS[name]
    ncrms, nx, nz = shape
    inp = inputs(oracle, name)
    c = [to_dev(a) for a in coeffs_of(name, 30)]

    def code(fn, *a, **kw):
        with pytest.raises(M.MpdataError) as e:
            fn(*a, **kw)
        return e.value.code

    p = new_plan(M, name)
    assert code(p.vsolve, *c) == M.ESTATE                                        # never filled
    upload(p, inp)
    before = whole(M, p, name)
    L = M.lib()
    ptr = [a.data_ptr() for a in c]
    raw = lambda sl0, n, first, ntr, a=ptr: L.mpdata_plan_vsolve_device(p._p, sl0, n, a[0], a[1], a[2], first, ntr)
    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, ncrms + 1), (ncrms, 1), (3, 3)):
        assert raw(sl0, n, 0, 1) == M.EINVAL, (sl0, n)
    for first, ntr in ((0, 0), (-1, 1), (2, 2), (3, 1), (0, 4)):
        assert raw(0, ncrms, first, ntr) == M.EINVAL, (first, ntr)
    for i, nm in enumerate(("lo", "di", "up")):
        a = list(ptr)
        a[i] = None
        assert raw(0, ncrms, 0, 1, a) == M.EINVAL and b"null " + nm.encode() in L.mpdata_last_error()
        assert raw(0, 0, 0, 1, a) == M.EINVAL and b"n = 0" in L.mpdata_last_error()                # the range first
        assert raw(0, ncrms, 0, 4, a) == M.EINVAL and b"tracer range" in L.mpdata_last_error()     # then the tracers
    # a host form of the other precision; its NULL comes first
    h32 = [np.asfortranarray(a.astype(F32)) for a in coeffs_of(name, 30)]
    assert L.mpdata_plan_vsolve_f32(p._p, 0, ncrms, *(a.ctypes.data for a in h32)) == M.ESTATE
    assert L.mpdata_plan_vsolve_f32(p._p, 0, ncrms, h32[0].ctypes.data, None, h32[2].ctypes.data) == M.EINVAL
    assert b"null di" in L.mpdata_last_error()
    after = whole(M, p, name)
    for k in before:
        assert_bitwise(after[k], before[k], f"after the refused calls: {k}")
    p.vsolve(*c)                                                                 # ... and the plan still works
    p.sync()
    assert not np.array_equal(whole(M, p, name, ("f",))["f"], before["f"])
    p.close()


# ---- 5. a multi-GPU handle is refused; the single-device plans of its shards take the call
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
        p.vsolve(*(to_dev(a) for a in c))
    assert e.value.code == M.EUNSUPPORTED and b"mpdata_plan_shard_plan" in M.lib().mpdata_last_error()
    with pytest.raises(M.MpdataError) as e:
        p.vsolve_host(*c)
    assert e.value.code == M.EUNSUPPORTED
    same_as_model(M, p, name, m, "after the refused handle calls")
    for g, (_, s0, nloc) in enumerate(p.shards()):
        q = p.shard_plan(g)
        cg = coeffs_of(name, 41 + g, nloc)
        vsolve(M, q, name, cg, 0, nloc, 0, T, call=q.vsolve)
        assert m.vsolve(*cg, sl0=s0, n=nloc) is None
        q.close()
    same_as_model(M, p, name, m, "after the shard plans' calls")
    p.run()
    assert m.run() is None
    same_as_model(M, p, name, m, "after the shard plans' calls and a run")
    p.close()


# ---- 6. the Fortran program: every record of its dump against the model
FORTRAN = {
    "f64": (F64, "vsolve_calls", (7, 5, 10), 3, (2, 3), (1, 2)), "f32": (F32, "vsolve_calls_sp", (6, 5, 10), 3, (1, 3), (1, 2)),
    "f64-whole": (F64, "vsolve_calls", (5, 3, 28), 2, (0, 5), (0, 2)), "f32-odd-ref": (F32, "vsolve_calls_sp", (7, 3, 12), 2, (6, 1), (1, 1)),
    "f64-nz72": (F64, "vsolve_calls", (3, 2, 72), 1, (1, 2), (0, 1)), "f32-nz72": (F32, "vsolve_calls_sp", (4, 2, 72), 2, (1, 2), (0, 2)),
}


@pytest.mark.parametrize("case", list(FORTRAN))
def test_fortran_program_matches_the_model(oracle, tmp_path, case):
    dt, exe, shape, T, (sl0, n), (t1, tn) = FORTRAN[case]
    ncrms, nx, nz = shape
    inp = VM.make_plan_inputs(oracle, shape, T, dt, SEED + 3)
    arrs = {k: (inp[k].reshape(inp[k].shape + (1,), order="F") if T == 1 and k in ("f", "flux") else inp[k]) for k in PM.NAMES}
    ca, cb = VM.make_coeffs(n, nz, dt, 700), VM.make_coeffs(ncrms, nz, dt, 701)
    records = [("params", np.array([ncrms, nx, nz, T, sl0, n, t1, tn], np.int64))]
    records += [(k, arrs[k]) for k in PM.NAMES]
    records += [(k + "_a", a) for k, a in zip(("lo", "di", "up"), ca)] + [(k + "_b", a) for k, a in zip(("lo", "di", "up"), cb)]
    # the replay on the model
    m = VM.PlanModelVsolve(oracle, ncrms, nx, nz, T, dt)
    want = FR.want_import(m, inp)
    rc = lambda what, code=None: want.append(FR.rc(what, code))
    rc("vs_block", m.vsolve(*ca, sl0=sl0, n=n)); rc("sync")
    e = m.export_device()
    rc("export"); rc("sync")
    want += [("f_a", e["f"]), ("flux_a", e["flux"])]
    rc("vs_range", m.vsolve(*cb, first=t1, ntr=tn)); rc("sync")
    want += FR.want_close(m)
    FR.compare_dump(FR.run_program(exe, records, tmp_path), want, case)
