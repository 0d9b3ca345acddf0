"""GPU tests of the large-scale vertical advection of a resident plan (include/mpdata_hip.h 3m):
mpdata_plan_subside_device, the host forms, the array forms, their Python face Plan.subside / subside_host /
subside_device, and the Fortran program tests/fortran/subside_calls.F90.

Every comparison is bit for bit (util.assert_bitwise) against the numpy model of tests/subside_model.py: SM.subside on a
reference-layout truth -- f with all its halo columns, and dsum --, or the plan model with the new call
(SM.PlanModelSubside: an EXACT plan's f and flux are bit-identical to it), or, for FAST plans, the plan's own whole export
before the call.  dsum lies inside a larger buffer with a patterned band of 4 KiB on both sides; the bands must come
back unchanged, and so must cb and cc.  cb, cc are random, of both signs, another value per instance and level; f is the
oracle's raw field moved by one half, so signed.

Shapes (ncrms, nx, nz): the smallest at which a path of the kernels differs.  (5, 3, 8): padding slots of an 8-instance
tile; (6, 4, 12); (5, 3, 28): element e +- 1 across the main / rest split and across instances in a wave; (3, 3, 64): 63
elements; (3, 2, 65), (3, 2, 72): element 63 | 64 across two waves; (2, 2, 140): three slices, an idle wave; (2, 2, 238):
four slices; (70, 3, 28) with 3 tracers: more than one workgroup.  fp32: pairs (even), the phantom (odd with the switch),
the reference layout (odd without it).  Windowed plans (nz > 238 with set_tall_columns): 239 and 300 levels, fp32 with 15
pseudo-instances (an inner phantom); 250 levels without the switch is a reference-layout plan."""
import numpy as np
import pytest

import fortran_records as FR
import plan_harness as H
import subside_model as SM
from oracle import plan_model as PM
from plan_harness import BAND, _defaults, banded, upload
from util import assert_bitwise, to_dev, to_host

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32

# name -> (shape, tracers, dtype, switches)
KINDS = {
    "f64-nz8": ((5, 3, 8), 2, F64, {}), "f64-nz12": ((6, 4, 12), 1, F64, {}), "f64-nz28": ((5, 3, 28), 2, F64, {}),
    "f64-nz64": ((3, 3, 64), 1, F64, {}), "f64-nz65": ((3, 2, 65), 1, F64, {}), "f64-nz72": ((3, 2, 72), 2, F64, {}),
    "f64-nz140": ((2, 2, 140), 1, F64, {}), "f64-nz238": ((2, 2, 238), 1, F64, {}), "f64-nz28-n70": ((70, 3, 28), 3, F64, {}),
    "f32-nz28-even": ((6, 3, 28), 2, F32, {}), "f32-nz72-even": ((4, 2, 72), 1, F32, {}),
    "f32-nz28-odd": ((7, 3, 28), 2, F32, dict(odd=True)), "f32-nz72-odd": ((3, 2, 72), 1, F32, dict(odd=True)),
    "f32-nz12-odd-ref": ((7, 3, 12), 1, F32, {}),      # (an odd fp32 plan without the switch keeps the reference layout)
    "f64-nz12-ref": ((5, 3, 12), 2, F64, dict(ref=True)), "f32-nz12-ref": ((6, 3, 12), 2, F32, dict(ref=True)),
    "f64-nz250-ref": ((2, 3, 250), 1, F64, {}),        # (above 238 levels without the switch: the reference layout)
    "f64-nz239-tall": ((2, 3, 239), 2, F64, dict(tall=True)), "f64-nz300-tall": ((3, 2, 300), 1, F64, dict(tall=True)),
    "f32-nz239-tall-odd": ((3, 2, 239), 2, F32, dict(tall=True, odd=True)),
}
REF = ("f32-nz12-odd-ref", "f64-nz12-ref", "f32-nz12-ref", "f64-nz250-ref")
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
    m = SM.PlanModelSubside(oracle, *shape, T, dt)
    assert m.upload({k: np.array(v, order="F") for k, v in inputs(oracle, name).items()}) is None
    return m


def whole(M, p, name, what=("f", "flux")):
    return H.whole(M, p, KINDS[name], what)


def same_as_model(M, p, name, m, what):
    H.same_as_model(M, p, KINDS[name], name, m, what)


def coeffs(name, k, n=None):
    shape, T, dt, _ = KINDS[name]
    return SM.make_coeffs(shape[0] if n is None else n, shape[2], dt, 500 + k)


def subside(M, p, name, c, sl0=0, n=None, first=0, ntr=None, dsum=True, lead=None):
    """Plan.subside of host coefficients c = (cb, cc) -> dsum (n, nzm, ntr) or None; cb, cc and the bands of dsum are checked"""
    import torch
    shape, T, dt, _ = KINDS[name]
    n = shape[0] - sl0 if n is None else n
    ntr = T - first if ntr is None else ntr
    dev = [to_dev(v) for v in c]
    orig = [v.clone() for v in dev]
    lead = (ntr != 1) if lead is None else lead
    db = banded(((ntr,) if lead else ()) + (shape[2] - 1, n), dt) if dsum else None
    torch.cuda.synchronize()      # (the plan may run on a stream that does not wait for the one that filled the buffers)
    p.subside(dev[0], dev[1], db[2] if dsum else None, sl0, n, first, ntr)
    p.sync()
    for v, o in zip(dev, orig):
        assert torch.equal(v, o), "a coefficient changed"
    if not dsum:
        return None
    raw, pristine, view = db
    assert torch.equal(raw[:BAND], pristine[:BAND]) and torch.equal(raw[-BAND:], pristine[-BAND:]), "dsum: a band byte changed"
    return to_host(view).reshape((n, shape[2] - 1, ntr), order="F")


# ---- 1. every kind of plan: whole plan, every state
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
    # (a) upload -> subside with dsum -> the model on the uploaded f, halo columns included (they differ from the interior)
    c0 = coeffs(name, 0)
    assert (c0[0] < 0).any() and (c0[0] > 0).any() and (c0[1] < 0).any() and (c0[1] > 0).any()
    assert not np.array_equal(F0[:, 2], F0[:, 3]) and (F0 < 0).any() and (F0 > 0).any()
    d = subside(M, p, name, c0)
    want_f, want_d = SM.subside(F0, *c0)
    assert not np.array_equal(want_f[:, :3], F0[:, :3])                  # (the halo columns move)
    assert_bitwise(d, want_d, f"{name} (a): dsum")
    assert_bitwise(d, m.subside(*c0), f"{name} (a): dsum of the plan model")
    got = whole(M, p, name)
    assert_bitwise(got["f"], want_f, f"{name} (a): f")
    assert_bitwise(got["flux"], inp["flux"].reshape(got["flux"].shape, order="F"), f"{name} (a): flux")
    # (b) a run on the kept velocities = export -> model -> import -> run: halos, seams and the phantom are consistent
    p.run()
    assert m.run() is None
    same_as_model(M, p, name, m, "(b) subside, run")
    # (c) behind the run (a windowed plan's seams are stale): subside without dsum, export, run
    c1 = coeffs(name, 1)
    assert subside(M, p, name, c1, dsum=False) is None
    assert m.subside(*c1) is not None
    same_as_model(M, p, name, m, "(c) run, subside")
    p.run()
    assert m.run() is None
    same_as_model(M, p, name, m, "(c) run, subside, run")
    # (d) PERIODIC: run, subside while the halos are stale, export = wrap(model)
    p.set_boundary(M.BOUNDARY_PERIODIC)
    assert m.set_boundary(PM.PERIODIC) is None
    p.run()
    assert m.run() is None
    c2 = coeffs(name, 2)
    d = subside(M, p, name, c2)
    assert_bitwise(d, m.subside(*c2), f"{name} (d) periodic, stale halos: dsum")
    same_as_model(M, p, name, m, "(d) periodic: run, subside on stale halos")
    # ... right after an import, then on the halos the export wrapped: they stay wrapped copies; then a run
    upload(p, inp)
    assert m.upload({k: np.array(v, order="F") for k, v in inp.items()}) is None
    c3 = coeffs(name, 3)
    d = subside(M, p, name, c3)
    assert_bitwise(d, m.subside(*c3), f"{name} (d) periodic, after an import: dsum")
    same_as_model(M, p, name, m, "(d) periodic: import, subside")
    d = subside(M, p, name, c1)
    assert_bitwise(d, m.subside(*c1), f"{name} (d) periodic, wrapped halos: dsum")
    p.run()
    assert m.run() is None
    same_as_model(M, p, name, m, "(d) periodic: subside on wrapped halos, run")
    p.close()
    # FAST: the same bits as EXACT on the uploaded f; after a run against the plan's own export changed by the model
    p = new_plan(M, name, variant=M.VARIANT_FAST)
    upload(p, inp)
    d = subside(M, p, name, c0)
    assert_bitwise(d, want_d, f"{name} FAST: dsum")
    assert_bitwise(whole(M, p, name, ("f",))["f"], want_f, f"{name} FAST upload, subside")
    p.run()
    E = whole(M, p, name, ("f",))["f"]
    d = subside(M, p, name, c1)
    want_E, want_dE = SM.subside(E, *c1)
    assert_bitwise(d, want_dE, f"{name} FAST run, subside: dsum")
    assert_bitwise(whole(M, p, name, ("f",))["f"], want_E, f"{name} FAST run, subside")
    p.close()


# ---- 2. blocks and tracer sub-ranges: what lies outside keeps every bit
BLOCKS = {
    # eight instances per tile, five instances: inside the tile, one instance, the last one
    "f64-nz8": [(1, 3), (2, 1), (4, 1), (0, 5)],
    # two per tile: mid-tile to mid-tile, the last (half-filled) tile
    "f64-nz28": [(1, 3), (4, 1), (0, 4)],
    "f64-nz72": [(1, 1), (1, 2)],
    "f64-nz140": [(1, 1), (0, 1)],
    # more than one workgroup: from inside a tile across workgroups
    "f64-nz28-n70": [(3, 40), (69, 1), (9, 1)],
    # fp32 pairs: a block that splits pairs at both ends
    "f32-nz28-even": [(1, 3), (5, 1), (2, 2)],
    # fp32 pairs, odd plan of 7 (instance 6 shares its pair with the phantom): blocks that hold and miss instance 6
    "f32-nz28-odd": [(1, 2), (6, 1), (5, 2), (0, 6), (3, 3), (0, 7)],
    "f32-nz72-odd": [(2, 1), (1, 1), (0, 2)],
    "f32-nz12-odd-ref": [(1, 3), (6, 1)],
    "f64-nz12-ref": [(1, 3), (4, 1)],
    # windowed plans: each behind an import (the first) and behind a run (the others: stale seams), a block and the whole
    "f64-nz239-tall": [(1, 1), (0, 1), (0, 2)],
    "f64-nz300-tall": [(1, 2), (0, 3), (2, 1)],
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
        c = coeffs(name, 10 + k, n)
        d = subside(M, p, name, c, sl0, n, first, ntr, lead=bool(k % 2) or ntr > 1)
        want_d = m.subside(*c, sl0=sl0, n=n, first=first, ntr=ntr)
        assert_bitwise(d, want_d, f"{name} block {sl0, n} tracers {first, ntr}: dsum")
        after = whole(M, p, name)
        out = np.ones(ncrms, bool)
        out[sl0:sl0 + n] = False
        tout = np.ones(T, bool)
        tout[first:first + ntr] = False
        assert_bitwise(after["f"][out], before["f"][out], f"{name} block {sl0, n}: instances outside")
        assert_bitwise(after["f"][..., tout], before["f"][..., tout], f"{name} block {sl0, n}: tracers outside")
        assert_bitwise(after["flux"], before["flux"], f"{name} block {sl0, n}: flux")
        want = SM.subside(before["f"][sl0:sl0 + n, ..., first:first + ntr], *c)[0]
        assert_bitwise(after["f"][sl0:sl0 + n, ..., first:first + ntr], want, f"{name} block {sl0, n}: inside")
        assert not np.array_equal(want, before["f"][sl0:sl0 + n, ..., first:first + ntr])
        # a run of every instance (the phantom of an odd plan rides with instance ncrms - 1; a windowed plan refreshes
        # the seams the call marked stale) matches the model
        p.run()
        assert m.run() is None
        same_as_model(M, p, name, m, f"block {sl0, n}, run")
    p.close()


# ---- 3. the host form and the array forms
@pytest.mark.parametrize("name", ["f64-nz28", "f32-nz28-odd", "f64-nz12-ref", "f64-nz72", "f64-nz239-tall"])
def test_host_form(mpdata, oracle, name):
    M = mpdata
    shape, T, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    p = new_plan(M, name)
    upload(p, inputs(oracle, name))
    m = model_of(oracle, name)
    for sl0, n, wd in ((0, ncrms, True), (1, 1, False), (ncrms - 1, 1, True)):
        c = coeffs(name, 20 + sl0, n)
        d = np.full((n, nz - 1) + ((T,) if T > 1 else ()), -7, dt, order="F") if wd else None
        p.subside_host(c[0], c[1], d, sl0, n)
        want_d = m.subside(*c, sl0=sl0, n=n)
        if wd:
            assert_bitwise(d.reshape(want_d.shape, order="F"), want_d, f"{name} host {sl0, n}: dsum")
        same_as_model(M, p, name, m, f"host form {sl0, n}")
        p.run()
        assert m.run() is None
        same_as_model(M, p, name, m, f"host form {sl0, n}, run")
    with pytest.raises(M.MpdataError):
        p.subside_host(c[0][:, :-1], c[1], sl0=ncrms - 1, n=1)       # a wrong shape
    p.close()


# 257 and 600 instances: more than one block of 256 threads and a partly filled last one; (2, 1, 3) with 32769 tracers:
# 65538 rows, the second trip over gridDim.y.  f and the coefficients are random, so instance b differs from b - 256 and
# row r from r - 65535.
ARRAYS = {"n257": ((257, 3, 6), 2), "n600": ((600, 2, 5), 1), "rows65538": ((2, 1, 3), 32769)}


@pytest.mark.parametrize("case", list(ARRAYS))
@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
def test_array_forms(mpdata, dt, case):
    import torch
    M = mpdata
    (ncrms, nx, nz), T = ARRAYS[case]
    rng = np.random.default_rng([77, ncrms, T])
    f = np.asfortranarray(rng.uniform(-1.0, 1.0, (ncrms, nx + 6, nz - 1, T)).astype(dt))
    cb, cc = SM.make_coeffs(ncrms, nz, dt, 600)
    want, want_d = SM.subside(f, cb, cc)
    if ncrms > 256:
        assert not np.array_equal(want[256:], want[:ncrms - 256]) and not np.array_equal(want_d[256:], want_d[:ncrms - 256])
    if T > 65535:
        rows = want.reshape((ncrms, nx + 6, -1), order="F")
        assert not np.array_equal(rows[..., 65535:], rows[..., :rows.shape[-1] - 65535])
    fd = to_dev(f)
    db = banded((T, nz - 1, ncrms), dt)
    torch.cuda.synchronize()
    M.subside_device(fd, to_dev(cb), to_dev(cc), db[2])
    torch.cuda.synchronize()
    raw, pristine, view = db
    assert torch.equal(raw[:BAND], pristine[:BAND]) and torch.equal(raw[-BAND:], pristine[-BAND:])
    assert_bitwise(to_host(fd), want, f"array form {case}: f")
    assert_bitwise(to_host(view), want_d, f"array form {case}: dsum")
    if T == 1 or case == "n257":
        # one tracer without the tracer axis, dsum skipped
        f1 = to_dev(np.asfortranarray(f[..., 0]))
        M.subside_device(f1, to_dev(cb), to_dev(cc))
        torch.cuda.synchronize()
        assert_bitwise(to_host(f1), want[..., 0], f"array form {case}, one tracer: f")


# ---- 4. every error code; the plan's state before and after
def test_errors_change_nothing(mpdata, oracle):
    M = mpdata
    name = "f64-nz28"
    shape, T, dt, _ = KINDS[name]
    ncrms, nx, nz = shape
    inp = inputs(oracle, name)
    c = coeffs(name, 30)
    dev = [to_dev(v) for v in c]

    def code(fn, *a, **kw):
        with pytest.raises(M.MpdataError) as e:
            fn(*a, **kw)
        return e.value.code

    p = new_plan(M, name)
    assert code(p.subside, *dev) == M.ESTATE                                     # never filled
    upload(p, inp)
    before = whole(M, p, name)
    L = M.lib()
    ptr = dict(cb=dev[0].data_ptr(), cc=dev[1].data_ptr())
    raw = lambda sl0, n, first, ntr, **kw: L.mpdata_plan_subside_device(p._p, sl0, n, kw.get("cb", ptr["cb"]), kw.get("cc", ptr["cc"]),
                                                                       None, first, ntr)
    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, ncrms + 1), (ncrms, 1), (3, 3)):
        assert raw(sl0, n, 0, 1) == M.EINVAL, (sl0, n)
    for first, ntr in ((0, 0), (-1, 1), (1, 2), (2, 1), (0, 3)):
        assert raw(0, ncrms, first, ntr) == M.EINVAL, (first, ntr)
    for k in ("cb", "cc"):
        assert raw(0, ncrms, 0, 1, **{k: None}) == M.EINVAL, k
        assert b"null " + k.encode() in L.mpdata_last_error()
    assert raw(0, 0, 0, 1, cb=None) == M.EINVAL and b"n = 0" in L.mpdata_last_error()             # the range first
    assert raw(0, ncrms, 0, 3, cb=None) == M.EINVAL and b"tracer range" in L.mpdata_last_error()  # then the tracers
    # a host form of the other precision
    c32 = [np.asfortranarray(v.astype(F32)) for v in c]
    assert L.mpdata_plan_subside_f32(p._p, 0, ncrms, c32[0].ctypes.data, c32[1].ctypes.data, None) == M.ESTATE
    after = whole(M, p, name)
    for k in before:
        assert_bitwise(after[k], before[k], f"after the refused calls: {k}")
    p.subside(*dev)                                                              # ... and the plan still works
    p.sync()
    assert not np.array_equal(whole(M, p, name, ("f",))["f"], before["f"])
    p.close()


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
    with pytest.raises(M.MpdataError) as e:
        p.subside(to_dev(c[0]), to_dev(c[1]))
    assert e.value.code == M.EUNSUPPORTED and b"mpdata_plan_shard_plan" in M.lib().mpdata_last_error()
    with pytest.raises(M.MpdataError) as e:
        p.subside_host(c[0], c[1])
    assert e.value.code == M.EUNSUPPORTED
    same_as_model(M, p, name, m, "after the refused handle calls")
    for g, (_, s0, nloc) in enumerate(p.shards()):
        q = p.shard_plan(g)
        cg = coeffs(name, 41 + g, nloc)
        d = subside(M, q, name, cg, 0, nloc)
        assert_bitwise(d, m.subside(*cg, sl0=s0, n=nloc), f"shard {g}: dsum")
        q.close()
    same_as_model(M, p, name, m, "after the shard plans' calls")
    p.run()
    assert m.run() is None
    same_as_model(M, p, name, m, "after the shard plans' calls and a run")
    p.close()


# ---- 6. the Fortran program: every record of its dump against the model
FORTRAN = {"f64": (F64, "subside_calls", (7, 5, 10), 3, (2, 3), (1, 2)), "f32": (F32, "subside_calls_sp", (6, 5, 10), 3, (1, 3), (1, 2))}


@pytest.mark.parametrize("case", list(FORTRAN))
def test_fortran_program_matches_the_model(oracle, tmp_path, case):
    dt, exe, shape, T, (sl0, n), (t1, tn) = FORTRAN[case]
    ncrms, nx, nz = shape
    inp = SM.make_plan_inputs(oracle, shape, T, dt, SEED + 3)
    cb_a, cc_a = SM.make_coeffs(n, nz, dt, 700)
    cb_b, cc_b = SM.make_coeffs(ncrms, nz, dt, 701)
    records = [("params", np.array([ncrms, nx, nz, T, sl0, n, t1, tn], np.int64))]
    records += [(k, inp[k]) for k in PM.NAMES] + [("cb_a", cb_a), ("cc_a", cc_a), ("cb_b", cb_b), ("cc_b", cc_b)]
    # the replay on the model
    m = SM.PlanModelSubside(oracle, ncrms, nx, nz, T, dt)
    want = FR.want_import(m, inp)
    rc = lambda what, code=None: want.append(FR.rc(what, code))
    dsum = m.subside(cb_a, cc_a, sl0=sl0, n=n)
    rc("subside_block"); rc("sync")
    want.append(("dsum", dsum))
    assert m.subside(cb_b, cc_b, first=t1, ntr=tn) is not None
    rc("subside_range"); rc("sync")
    want += FR.want_close(m)
    FR.compare_dump(FR.run_program(exe, records, tmp_path), want, case)
