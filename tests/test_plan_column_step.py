"""GPU tests of the fused column step of a resident plan (include/mpdata_hip.h 3q): mpdata_plan_column_step_device, the host
forms, the array forms, their Python face Plan.column_step_device / column_step / column_step_device, and the Fortran
program tests/fortran/column_step_calls.F90.

Every comparison is bit for bit (util.assert_bitwise) against the numpy model of tests/column_step_model.py, which composes
the models of the single sections 3p, 3m, 3n, 3o: QM.column_step on a reference-layout truth, or the plan model with the
new call (QM.PlanModelColumnStep: an EXACT plan's f and flux are bit-identical to it), or, for FAST plans, the plan's own
whole export before the call.  Every input array -- s, wp, cb, cc, lo, di, up -- lies inside a larger buffer with 4 KiB of
NaN on both sides, so a read outside the block's array poisons the result, and must come back unchanged; psfc is filled
with NaN and lies between two patterned bands of 4 KiB, which must come back unchanged.  The inputs are those of the
single sections' tests (make_s, make_coeffs, make_wp); f is the oracle's raw field moved by one half, so signed and without
-0.0; c = 0.75, and 0.1 -- no fp32 number, the library rounds it once -- on the kind "f32-nz28-even".  A call clips where
it meets the uploaded field, which is symmetric about zero, and then asserts ON THE MODEL that the clip acts on 20 % ..
80 % of the touched cells, so that the later stages see clipped values; behind a clipped call the field is no longer
symmetric, and the calls that follow add without the clip.

The kinds are those of tests/test_plan_cell_add.py without the tall ones: the smallest shapes at which this staging can go
wrong -- many slots per tile (nz = 8: a group of 32 units), nx no multiple of the column batch (nx = 11), three groups
with a ragged last one, two and more slices per tile (nz = 65, 72, 140, 238: the group shrinks until a column fits the
LDS), fp32 pairs, the phantom of an odd fp32 plan, and the reference layout in its four ways."""
import numpy as np
import pytest

import cell_add_model as CM
import column_step_model as QM
import fortran_records as FR
import plan_harness as H
from oracle import plan_model as PM
from plan_harness import BAND, _defaults, nan_banded, nan_out, upload
from test_plan_cell_add import FAST as FAST_ALL
from test_plan_cell_add import KINDS as KINDS_ALL
from test_plan_cell_add import PERIODIC as PERIODIC_ALL
from test_plan_cell_add import REF, G, factor, inputs, same, snap
from util import assert_bitwise, to_dev, to_host

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
KINDS = {k: v for k, v in KINDS_ALL.items() if not v[3].get("tall")}
FAST = tuple(k for k in FAST_ALL if k in KINDS)
PERIODIC = tuple(k for k in PERIODIC_ALL if k in KINDS) + ("f32-nz28-even",)
ADD, CLIP = QM.ADD, QM.CLIP
ORDER = ("s", "cb", "cc", "wp", "lo", "di", "up")


def new_plan(M, name, variant=None):
    return H.new_plan(M, KINDS[name], name, name in REF, False, variant)


def whole(M, p, name, what=("f", "flux")):
    return H.whole(M, p, KINDS[name], what)


def test_the_kinds_and_their_runs():
    assert len(KINDS) == 17 and len(PERIODIC) == 4 and len(FAST) == 4


def model_of(oracle, name, inp=None):
    shape, T, dt, _ = KINDS[name]
    m = QM.PlanModelColumnStep(oracle, *shape, T, dt)
    assert m.upload({k: np.array(v, order="F") for k, v in (inp or inputs(oracle, name)).items()}) is None
    return m


def args_of(name, k, n=None, ntr=None, stages=QM.STAGES):
    """the arrays of a call on a block of KINDS[name], another set per k; s and wp with a tracer axis"""
    shape, T, dt, _ = KINDS[name]
    return QM.make_args(shape[0] if n is None else n, shape[1], shape[2], T if ntr is None else ntr, dt, 900 + 10 * k, stages)


def step(M, dims, dt, kw, c, mode, sl0=0, n=None, first=0, ntr=None, psfc=True, lead=None, call=None, sync=None):
    """call(...) = Plan.column_step_device of host arrays kw -> psfc (n, nx, ntr) or None; the inputs and the bands are
    checked.  dims: (ncrms, nx, nz, T) of the plan."""
    import torch
    ncrms, nx, nz, T = dims
    n = ncrms - sl0 if n is None else n
    ntr = T - first if ntr is None else ntr
    lead = (ntr != 1) if lead is None else lead
    sh = M.column_step_shapes(n, nx, nz, ntr if lead else None)
    dev, raws = {}, []
    for k in ORDER:
        if kw.get(k) is not None:
            assert kw[k].dtype == dt
            raw, dev[k] = nan_banded(kw[k], sh[k])
            raws.append((k, raw, raw.clone()))
    buf = nan_out(sh["psfc"], dt) if psfc and "wp" in dev else None
    torch.cuda.synchronize()      # (the plan may run on a stream that does not wait for the one that filled the buffers)
    call(c=c, mode=mode, psfc=buf[2] if buf else None, sl0=sl0, n=n, first_tracer=first, ntracers=ntr, **dev)
    if sync:
        sync()
    torch.cuda.synchronize()
    for k, raw, orig in raws:
        assert torch.equal(raw.view(torch.uint8), orig.view(torch.uint8)), f"{k} changed"
    if not buf:
        return None
    raw, pristine, view = buf
    assert torch.equal(raw[:BAND], pristine[:BAND]) and torch.equal(raw[-BAND:], pristine[-BAND:]), "psfc: a band byte changed"
    return to_host(view).reshape((n, nx, ntr), order="F")


def plan_step(M, p, name, kw, c, mode, **o):
    shape, T, dt, _ = KINDS[name]
    return step(M, shape + (T,), dt, kw, c, mode, call=o.pop("call", p.column_step_device), sync=p.sync, **o)


def model_step(m, kw, c, mode, sl0=0, n=None, first=0, ntr=None, psfc=True):
    """the call on the plan model -> psfc; under CLIP the clip condition is asserted first on the field the call meets"""
    ncrms, T = m.dims[0], m.dims[3]
    n = ncrms - sl0 if n is None else n
    ntr = T - first if ntr is None else ntr
    if mode == CLIP and kw.get("s") is not None:
        frac = CM.clipped_fraction(m.a["f"][sl0:sl0 + n, ..., first:first + ntr], kw["s"], c)
        assert 0.2 <= frac <= 0.8, (sl0, n, first, ntr, frac)
    ps = m.column_step(c=c, mode=mode, psfc=psfc and kw.get("wp") is not None, sl0=sl0, n=n, first=first, ntr=ntr, **kw)
    assert not isinstance(ps, int), ps
    return ps


# ---- 1. every kind of plan: the whole plan, all four stages and psfc, the first call clipped; a run behind every call
@pytest.mark.parametrize("name", list(KINDS))
def test_every_plan_kind(mpdata, oracle, name):
    M = mpdata
    shape, T, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    c = factor(name)
    inp = inputs(oracle, name)
    assert not np.any(np.signbit(inp["f"]) & (inp["f"] == 0))
    # ---- the model's pass: behind the upload, then behind a run, without psfc
    m = model_of(oracle, name)
    want = []
    for k in (0, 1):
        before = np.array(m.a["f"], order="F")
        ps = model_step(m, args_of(name, k), c, ADD if k else CLIP, psfc=k == 0)
        assert_bitwise(m.a["f"][:, :3], before[:, :3], "the halos stay")
        assert_bitwise(m.a["f"][:, nx + 3:], before[:, nx + 3:], "the halos stay")
        assert not np.array_equal(m.a["f"], before)
        after = snap(m)
        assert m.run() is None
        want.append((ps, after, snap(m)))
    per = []
    if name in PERIODIC:
        assert m.set_boundary(PM.PERIODIC) is None and m.run() is None
        for k in (5, 6, 7, 8):
            ps = model_step(m, args_of(name, k), c, ADD)
            if k == 7:
                assert m.run() is None
            if k == 8:
                assert m.set_boundary(PM.GIVEN) is None
            per.append((ps, snap(m)))
    # ---- the plan's pass
    p = new_plan(M, name)
    upload(p, inp)
    for k, (wps, w_call, w_run) in zip((0, 1), want):
        got = plan_step(M, p, name, args_of(name, k), c, ADD if k else CLIP, psfc=k == 0)
        if k == 0:
            assert_bitwise(got, wps, f"{name} call {k}: psfc")
        same(whole(M, p, name), w_call, f"{name} call {k}")
        p.run()                   # (the phantom of an odd plan rides with instance ncrms - 1; u, w, rho, rhow, adz enter it)
        same(whole(M, p, name), w_run, f"{name} call {k}, run")
    if name in PERIODIC:
        p.set_boundary(M.BOUNDARY_PERIODIC)
        p.run()
        # (5) the halos are stale behind the run; the export hands out wrapped halos of the NEW field   (6) on halos the
        # export just wrapped   (7) a run right behind the call, no read-back between   (8) back to GIVEN behind a call
        for k, (wps, w) in zip((5, 6, 7, 8), per):
            got = plan_step(M, p, name, args_of(name, k), c, ADD)
            assert_bitwise(got, wps, f"{name} periodic {k}: psfc")
            if k == 7:
                p.run()
            if k == 8:
                p.set_boundary(M.BOUNDARY_GIVEN)
            e = whole(M, p, name)
            same(e, w, f"{name} periodic {k}")
            if k in (5, 6):
                assert_bitwise(e["f"], PM.wrap(np.array(e["f"], order="F")), f"{name} periodic {k}: wrapped copies of the new interior")
    p.close()
    if name in FAST:
        # FAST: the same bits as EXACT on the uploaded f; after a run against the plan's own export changed by the model
        p = new_plan(M, name, variant=M.VARIANT_FAST)
        upload(p, inp)
        assert_bitwise(plan_step(M, p, name, args_of(name, 0), c, CLIP), want[0][0], f"{name} FAST: psfc")
        assert_bitwise(whole(M, p, name, ("f",))["f"], want[0][1]["f"], f"{name} FAST upload, column_step")
        p.run()
        E = whole(M, p, name, ("f",))["f"]
        kw = args_of(name, 1)
        got = plan_step(M, p, name, kw, c, ADD)
        rho, adz = (np.asarray(inp[k]).reshape((ncrms, nz - 1), order="F") for k in ("rho", "adz"))
        want_E, want_ps = QM.column_step(E, rho, adz, c=c, mode=ADD, **kw)
        assert_bitwise(got, want_ps, f"{name} FAST run, column_step: psfc")
        assert_bitwise(whole(M, p, name, ("f",))["f"], want_E, f"{name} FAST run, column_step")
        p.close()


# ---- 2. every set of stages, against the model AND against the sequence of the single calls on a second plan
@pytest.mark.parametrize("stages", QM.SUBSETS, ids=["+".join(s) for s in QM.SUBSETS])
@pytest.mark.parametrize("name", ["f64-nz28-nx11", "f32-nz28-odd"])
def test_every_set_of_stages(mpdata, oracle, name, stages):
    M = mpdata
    shape, T, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    c = 0.75
    inp = inputs(oracle, name)
    kw = args_of(name, 3, stages=stages)
    m = model_of(oracle, name)
    wps = model_step(m, kw, c, CLIP)
    w_call = snap(m)
    assert m.run() is None
    p, q = new_plan(M, name), new_plan(M, name)
    upload(p, inp)
    upload(q, inp)
    got = plan_step(M, p, name, kw, c, CLIP)
    d = {k: to_dev(v) for k, v in kw.items()}
    ps_q = None
    if "source" in stages:
        q.cell_add(d["s"], c, CLIP)
    if "subside" in stages:
        q.subside(d["cb"], d["cc"], ntracers=T)
    if "sediment" in stages:
        import torch
        ps_q = torch.empty(M.sediment_shapes(ncrms, nx, nz, T)["psfc"], dtype=d["wp"].dtype, device="cuda:0")
        q.sediment(d["wp"], ps_q)
    if "vsolve" in stages:
        q.vsolve(d["lo"], d["di"], d["up"], ntracers=T)
    q.sync()
    ep, eq = whole(M, p, name), whole(M, q, name)
    same(ep, w_call, f"{name} {stages}: the model")
    assert_bitwise(ep["f"][:, 3:nx + 3], eq["f"][:, 3:nx + 3], f"{name} {stages}: the sequence of the single calls, interior")
    assert_bitwise(ep["flux"], eq["flux"], f"{name} {stages}: flux")
    assert_bitwise(ep["f"][:, :3], inp["f"].reshape(ep["f"].shape, order="F")[:, :3], f"{name} {stages}: the halos keep every bit")
    if "sediment" in stages:
        assert_bitwise(got, wps, f"{name} {stages}: psfc")
        assert_bitwise(got, to_host(ps_q).reshape(got.shape, order="F"), f"{name} {stages}: psfc of the single call")
    else:
        assert got is None
    # the next run sees the same field: PERIODIC, so that 3m's halo slots of the sequence do not enter
    for x in (p, q):
        x.set_boundary(M.BOUNDARY_PERIODIC)
        x.run()
    same(whole(M, p, name), whole(M, q, name), f"{name} {stages}: a periodic run behind both")
    p.close()
    q.close()


# ---- 3. blocks and tracer sub-ranges: what lies outside keeps every bit
BLOCKS = {
    "f64-nz8": [(1, 3), (4, 1), (0, 5)],
    "f64-nz28-nx11": [(1, 3), (4, 1)],
    # three groups: a block across a group boundary, odd sl0 across two boundaries, the last instance alone
    "f64-nz28-3groups": [(G - 1, 3), (3, 2 * G), (2 * G + 4, 1)],
    "f64-nz140": [(1, 1), (0, 1)],
    # fp32 pairs: blocks that split pairs at both ends
    "f32-nz28-even": [(1, 3), (5, 1), (2, 2)],
    "f32-nz28-3groups": [(2 * G - 1, 3), (1, 4 * G + 4)],
    # an odd plan of 7 (instance 6 shares its pair with the phantom): blocks that hold and miss instance 6
    "f32-nz28-odd": [(1, 2), (6, 1), (5, 2), (0, 6)],
    "f32-nz72-odd": [(2, 1), (1, 1)],
    "f32-nz12-odd-ref": [(1, 3), (6, 1)],
    "f64-nz12-ref": [(1, 3), (4, 1)],
}
# the first block of these splits an fp32 pair: the instances next to it hold -0.0 and negative values, which stay
SPLIT = {"f32-nz28-even": (0, 4), "f32-nz28-3groups": (2 * G - 2, 2 * G + 2), "f32-nz28-odd": (0, 3)}


@pytest.mark.parametrize("name", list(BLOCKS))
def test_blocks_leave_the_rest_alone(mpdata, oracle, name):
    M = mpdata
    shape, T, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    c = factor(name)
    inp = dict(inputs(oracle, name))
    if name in SPLIT:
        f = np.array(inp["f"], order="F")
        for b in SPLIT[name]:
            f[b, 3, ::2] = -0.0
            assert (f[b, 3:nx + 3] < 0).any()
        inp["f"] = f
    calls = []
    for k, (sl0, n) in enumerate(BLOCKS[name]):
        first, ntr = ((k % T), 1) if T > 1 else (0, 1)
        if T > 1 and k == len(BLOCKS[name]) - 1:
            first, ntr = 0, T
        calls.append((k, sl0, n, first, ntr))
    m = model_of(oracle, name, inp)
    want = []
    for k, sl0, n, first, ntr in calls:
        before = snap(m)
        ps = model_step(m, args_of(name, 10 + k, n, ntr), c, ADD if k else CLIP, sl0, n, first, ntr)
        after = snap(m)
        assert not np.array_equal(after["f"][sl0:sl0 + n, ..., first:first + ntr], before["f"][sl0:sl0 + n, ..., first:first + ntr])
        assert m.run() is None
        want.append((ps, before, after, snap(m)))
    p = new_plan(M, name)
    upload(p, inp)
    for (k, sl0, n, first, ntr), (wps, w_before, w_after, w_run) in zip(calls, want):
        what = f"{name} block {sl0, n} tracers {first, ntr}"
        before = whole(M, p, name)
        same(before, w_before, what + ": before")
        got = plan_step(M, p, name, args_of(name, 10 + k, n, ntr), c, ADD if k else CLIP, sl0=sl0, n=n, first=first, ntr=ntr, lead=bool(k % 2) or ntr > 1)
        assert_bitwise(got, wps, what + ": psfc")
        after = whole(M, p, name)
        out = np.ones(ncrms, bool)
        out[sl0:sl0 + n] = False
        tout = np.ones(T, bool)
        tout[first:first + ntr] = False
        assert_bitwise(after["f"][out], before["f"][out], what + ": instances outside")
        assert_bitwise(after["f"][..., tout], before["f"][..., tout], what + ": tracers outside")
        assert_bitwise(after["f"][:, :3], before["f"][:, :3], what + ": halo columns")
        assert_bitwise(after["f"][:, nx + 3:], before["f"][:, nx + 3:], what + ": halo columns")
        assert_bitwise(after["flux"], before["flux"], what + ": flux")
        same(after, w_after, what + ": the call")
        if k == 0 and name in SPLIT:
            for b in SPLIT[name]:
                assert out[b] and np.all(np.signbit(after["f"][b, 3, ::2, first]) & (after["f"][b, 3, ::2, first] == 0)), b
                assert (after["f"][b, 3:nx + 3, :, first] < 0).any(), b
        p.run()
        same(whole(M, p, name), w_run, what + ": the call, run")
    p.close()


# ---- 4. the host form and the array forms
@pytest.mark.parametrize("name", ["f64-nz28-nx11", "f32-nz28-odd", "f64-nz12-ref", "f64-nz72"])
def test_host_form(mpdata, oracle, name):
    M = mpdata
    shape, T, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    c = factor(name)
    script = ((0, ncrms, QM.STAGES, True), (1, 1, ("source", "vsolve"), False), (ncrms - 1, 1, ("subside", "sediment"), True))
    m = model_of(oracle, name)
    want = []
    for k, (sl0, n, stages, psfc) in enumerate(script):
        ps = model_step(m, args_of(name, 20 + k, n, stages=stages), c, ADD if k else CLIP, sl0, n, psfc=psfc)
        after = snap(m)
        assert m.run() is None
        want.append((ps, after, snap(m)))
    p = new_plan(M, name)
    upload(p, inputs(oracle, name))
    for k, ((sl0, n, stages, psfc), (wps, w_call, w_run)) in enumerate(zip(script, want)):
        kw = args_of(name, 20 + k, n, stages=stages)
        keep = {a: np.array(v, order="F") for a, v in kw.items()}
        ps = np.full((n, nx, T), np.nan, dt, order="F") if psfc and "wp" in kw else None
        p.column_step(c=c, mode=ADD if k else CLIP, psfc=ps, sl0=sl0, n=n, **kw)
        for a in kw:
            assert_bitwise(kw[a], keep[a], f"{name} host {sl0, n}: {a}")
        if ps is not None:
            assert_bitwise(ps, wps, f"{name} host {sl0, n}: psfc")
        same(whole(M, p, name), w_call, f"{name} host form {sl0, n}")
        p.run()
        same(whole(M, p, name), w_run, f"{name} host form {sl0, n}, run")
    with pytest.raises(M.MpdataError):
        p.column_step(cb=kw["cb"][:, :-1], cc=kw["cc"], sl0=ncrms - 1, n=1)       # a wrong shape
    p.close()


# 257 and 600 instances: more than one block of 256 threads and a partly filled last one, each with a block inside the
# arrays (the leading dimension of f, rho, adz is larger than n); (2, 1, 3) with 32769 tracers and one column: 65538 rows, the
# second trip over gridDim.y
ARRAYS = {"n257": ((257, 3, 6), 2, (1, 256)), "n600": ((600, 2, 5), 1, (300, 299)), "rows65538": ((2, 1, 3), 32769, (1, 1))}


@pytest.mark.parametrize("case", list(ARRAYS))
@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
def test_array_forms(mpdata, dt, case):
    import torch
    M = mpdata
    (ncrms, nx, nz), T, (b0, bn) = ARRAYS[case]
    rng = np.random.default_rng([78, ncrms, T])
    f = np.asfortranarray(rng.uniform(-0.5, 0.5, (ncrms, nx + 6, nz - 1, T)).astype(dt))
    rho, adz = (np.asfortranarray(rng.uniform(0.5, 1.0, (ncrms, nz - 1)).astype(dt)) for _ in range(2))
    c = 0.1 if dt == F32 else 0.75
    for (sl0, n), stages in (((0, ncrms), QM.STAGES), ((b0, bn), QM.STAGES), ((b0, bn), ("source", "subside"))):
        kw = QM.make_args(n, nx, nz, T, dt, 600 + sl0, stages)
        assert 0.2 <= CM.clipped_fraction(f[sl0:sl0 + n], kw["s"], c) <= 0.8
        want, want_ps = QM.column_step(f[sl0:sl0 + n], rho[sl0:sl0 + n], adz[sl0:sl0 + n], c=c, mode=CLIP, **kw)
        full = np.array(f, order="F")
        full[sl0:sl0 + n] = want
        if n > 256:
            assert not np.array_equal(want[256:], want[:n - 256])
        if T > 32768:
            assert not np.array_equal(want[..., 32768:], want[..., :T - 32768])
        fd, rd, ad = to_dev(f), to_dev(rho), to_dev(adz)
        with_wp = "sediment" in stages
        got = step(M, (ncrms, nx, nz, T), dt, kw, c, CLIP, sl0, n, lead=True,
                   call=lambda first_tracer, ntracers, **o: M.column_step_device(fd, rd if with_wp else None, ad if with_wp else None, **o))
        torch.cuda.synchronize()
        assert_bitwise(to_host(fd), full, f"array form {case} block {sl0, n} {stages}: f")
        if with_wp:
            assert_bitwise(got, want_ps, f"array form {case} block {sl0, n}: psfc")
    if case == "n257":
        # one tracer without the tracer axis, psfc skipped
        f1 = to_dev(np.asfortranarray(f[..., 0]))
        kw = QM.make_args(ncrms, nx, nz, None, dt, 650)
        M.column_step_device(f1, to_dev(rho), to_dev(adz), c=c, **{k: to_dev(v) for k, v in kw.items()})
        torch.cuda.synchronize()
        assert_bitwise(to_host(f1), QM.column_step(f[..., 0], rho, adz, c=c, **kw)[0], f"array form {case}, one tracer: f")


# ---- 5. every error code, in the stated order; the plan's state before and after
def test_errors_change_nothing(mpdata, oracle):
    M = mpdata
    name = "f64-nz28-nx11"
    shape, T, dt, _ = KINDS[name]
    ncrms, nx, nz = shape
    inp = inputs(oracle, name)
    kw = args_of(name, 30, ntr=1)
    d = {k: to_dev(v[..., 0] if v.ndim == 4 else v) for k, v in kw.items()}
    P = {k: v.data_ptr() for k, v in d.items()}

    def code(fn, *a, **k2):
        with pytest.raises(M.MpdataError) as e:
            fn(*a, **k2)
        return e.value.code

    p = new_plan(M, name)
    assert code(p.column_step_device, **d) == M.ESTATE                              # never filled
    upload(p, inp)
    before = whole(M, p, name)
    L = M.lib()
    err = L.mpdata_last_error

    def raw(sl0=0, n=ncrms, first=0, ntr=1, mode=0, psfc=None, **o):
        a = dict(P)
        a.update(o)
        return L.mpdata_plan_column_step_device(p._p, sl0, n, a["s"], 0.75, mode, a["cb"], a["cc"], a["wp"], psfc, a["lo"], a["di"], a["up"],
                                                first, ntr)
    none = dict.fromkeys(ORDER)
    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, ncrms + 1), (ncrms, 1), (3, 3)):
        assert raw(sl0, n) == M.EINVAL, (sl0, n)
    for first, ntr in ((0, 0), (-1, 1), (1, 2), (2, 1), (0, 3)):
        assert raw(first=first, ntr=ntr) == M.EINVAL and b"tracer range" in err(), (first, ntr)
    assert raw(**none) == M.EINVAL and b"no stage" in err()
    assert raw(cc=None) == M.EINVAL and b"cb without cc" in err() and raw(cb=None) == M.EINVAL and b"cc without cb" in err()
    assert raw(up=None) == M.EINVAL and b"null up" in err() and raw(lo=None, di=None) == M.EINVAL and b"null lo" in err()
    assert raw(wp=None, psfc=P["s"]) == M.EINVAL and b"psfc without wp" in err()
    for mode in (2, -1):
        assert raw(mode=mode) == M.EINVAL and b"unknown mode" in err()
    assert raw(mode=2, s=None) == 0                                                 # the mode is ignored without s
    p.sync()
    upload(p, inp)
    assert raw(mode=2, cc=None) == M.EINVAL and b"cb without cc" in err()           # the NULLs before the mode
    assert raw(n=0, **none) == M.EINVAL and b"n = 0" in err()                       # the range first
    assert raw(ntr=3, **none) == M.EINVAL and b"tracer range" in err()              # then the tracers
    assert code(p.column_step_device, mode=2, **d) == M.EINVAL
    # a host form of the other precision; its NULLs and its mode come first
    h32 = {k: np.asfortranarray((v[..., 0] if v.ndim == 4 else v).astype(F32)) for k, v in kw.items()}
    H = {k: v.ctypes.data for k, v in h32.items()}
    h = lambda mode=0, **o: L.mpdata_plan_column_step_f32(p._p, 0, ncrms, *[dict(H, **o)[k] for k in ("s",)], 0.75, mode,
                                                          *[dict(H, **o)[k] for k in ("cb", "cc", "wp")], None,
                                                          *[dict(H, **o)[k] for k in ("lo", "di", "up")])
    assert h() == M.ESTATE
    assert h(**none) == M.EINVAL and b"no stage" in err() and h(mode=2) == M.EINVAL and h(di=None) == M.EINVAL
    after = whole(M, p, name)
    for k in before:
        assert_bitwise(after[k], before[k], f"after the refused calls: {k}")
    p.column_step_device(**d)                                                       # ... and the plan still works
    p.sync()
    assert not np.array_equal(whole(M, p, name, ("f",))["f"], before["f"])
    p.close()


def test_a_windowed_plan_is_refused(mpdata, oracle):
    M = mpdata
    shape, T, dt = (2, 3, 239), 1, F64
    M.set_tall_columns(1)
    p = M.Plan(*shape, T, dtype=dt)
    assert p.level_windows > 1
    inp = QM.make_plan_inputs(oracle, shape, T, dt, 100)
    upload(p, inp)
    sh = M.shapes(*shape, T)
    ex = lambda: {k: to_host(v) for k, v in _export(M, p, sh, dt).items()}
    before = ex()
    kw = QM.make_args(*shape, None, dt, 50)
    d = {k: to_dev(v) for k, v in kw.items()}
    for sub in (d, {"s": d["s"]}, {"lo": d["lo"], "di": d["di"], "up": d["up"]}):
        with pytest.raises(M.MpdataError) as e:
            p.column_step_device(**sub)
        assert e.value.code == M.EUNSUPPORTED and b"windowed" in M.lib().mpdata_last_error()
    with pytest.raises(M.MpdataError) as e:
        p.column_step(**kw)
    assert e.value.code == M.EUNSUPPORTED and b"windowed" in M.lib().mpdata_last_error()
    with pytest.raises(M.MpdataError) as e:
        p.column_step_device()                                                      # the NULLs come first
    assert e.value.code == M.EINVAL
    after = ex()
    for k in before:
        assert_bitwise(after[k], before[k], f"after the refused calls: {k}")
    p.cell_add(d["s"], 0.75)                                                        # the single calls serve it
    p.sync()
    assert not np.array_equal(ex()["f"], before["f"])
    p.close()


def _export(M, p, sh, dt):
    import torch
    t = {k: torch.empty(sh[k], dtype=torch.float64 if dt == F64 else torch.float32, device="cuda:0") for k in ("f", "flux")}
    p.export_device(**t)
    p.sync()
    return t


# ---- 6. a multi-GPU handle is refused; the single-device plans of its shards take the call
def test_multi_gpu_handle_and_shard_plan(mpdata, oracle, monkeypatch):
    M = mpdata
    monkeypatch.delenv("MPDATA_MULTI_XFER", raising=False)
    name = "f64-nz28-nx11"
    shape, T, dt, _ = KINDS[name]
    inp = inputs(oracle, name)
    p = M.Plan(*shape, T, dtype=dt, devices=[0, 0])
    upload(p, inp)
    m = model_of(oracle, name)
    kw = args_of(name, 40)
    with pytest.raises(M.MpdataError) as e:
        p.column_step_device(**{k: to_dev(v) for k, v in kw.items()})
    assert e.value.code == M.EUNSUPPORTED and b"mpdata_plan_shard_plan" in M.lib().mpdata_last_error()
    with pytest.raises(M.MpdataError) as e:
        p.column_step(**kw)
    assert e.value.code == M.EUNSUPPORTED
    same(whole(M, p, name), m.export_device(), "after the refused handle calls")
    for g, (_, s0, nloc) in enumerate(p.shards()):
        q = p.shard_plan(g)
        kg = args_of(name, 41 + g, nloc)
        want = model_step(m, kg, 0.75, CLIP, s0, nloc)
        got = step(M, (nloc,) + shape[1:] + (T,), dt, kg, 0.75, CLIP, 0, nloc, call=q.column_step_device, sync=q.sync)
        assert_bitwise(got, want, f"shard {g}: psfc")
        q.close()
    same(whole(M, p, name), m.export_device(), "after the shard plans' calls")
    p.run()
    assert m.run() is None
    same(whole(M, p, name), m.export_device(), "after the shard plans' calls and a run")
    p.close()


# ---- 7. the Fortran program: every record of its dump against the model
FORTRAN = {
    "f64": (F64, "column_step_calls", (7, 5, 10), 3, (2, 3), (1, 2)), "f32": (F32, "column_step_calls_sp", (6, 5, 10), 3, (1, 3), (1, 2)),
    "f64-whole": (F64, "column_step_calls", (5, 3, 28), 2, (0, 5), (0, 2)),
    "f32-odd-ref": (F32, "column_step_calls_sp", (7, 3, 12), 2, (6, 1), (1, 1)),
}


@pytest.mark.parametrize("case", list(FORTRAN))
def test_fortran_program_matches_the_model(oracle, tmp_path, case):
    """the program's factors: 0.75 clipped on the block, 0.1 (a double; the fp32 program's plan rounds it once) on the range"""
    dt, exe, shape, T, (sl0, n), (t1, tn) = FORTRAN[case]
    ncrms, nx, nz = shape
    inp = QM.make_plan_inputs(oracle, shape, T, dt, 103)
    arrs = {k: (inp[k].reshape(inp[k].shape + (1,), order="F") if T == 1 and k in ("f", "flux") else inp[k]) for k in PM.NAMES}
    ka = QM.make_args(n, nx, nz, T, dt, 700)
    kb = QM.make_args(ncrms, nx, nz, tn, dt, 710, ("source", "vsolve"))
    records = [("params", np.array([ncrms, nx, nz, T, sl0, n, t1, tn], np.int64))]
    records += [(k, arrs[k]) for k in PM.NAMES] + [("s_a", ka["s"]), ("s_b", kb["s"]), ("wp", ka["wp"]), ("cb", ka["cb"]), ("cc", ka["cc"])]
    records += [("lo_a", ka["lo"]), ("di_a", ka["di"]), ("up_a", ka["up"]), ("lo_b", kb["lo"]), ("di_b", kb["di"]), ("up_b", kb["up"])]
    # the replay on the model
    m = QM.PlanModelColumnStep(oracle, ncrms, nx, nz, T, dt)
    want = FR.want_import(m, inp)
    rc = lambda what, code=None: want.append(FR.rc(what, code))
    psfc = model_step(m, ka, 0.75, CLIP, sl0, n)
    rc("step_block"); rc("sync")
    want += [("psfc", psfc)]
    model_step(m, kb, 0.1, ADD, first=t1, ntr=tn)
    rc("step_range"); rc("sync")
    rc("step_none", m.column_step())
    want += FR.want_close(m)
    FR.compare_dump(FR.run_program(exe, records, tmp_path), want, case)
