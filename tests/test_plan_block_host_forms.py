"""GPU tests of the two forms of the seven calls on a block of instances of a resident plan (include/mpdata_hip.h 3g .. 3m:
level statistics, Courant number, level increments, velocity scaling, column integrals, eddy diffusion, subsidence).

1. Optional arrays.  The host form stages its arrays on the device in argument order, and an absent optional array takes
   no room, so where the others lie depends on which are given.  For every subset of the optional arrays a call allows,
   the host form on one plan is compared bit for bit (util.assert_bitwise) with the device form, given the same arrays, on
   an identical second plan: the outputs, and for the calls that rewrite the plan its whole state afterwards -- f and flux
   by a download, u and w through the Courant number of the whole plan.
2. Check order.  Calls that break two rules at once must report the earlier one, by error code and by the text of
   mpdata_last_error(): the block, the tracer range, the call's own arguments (NULLs, the mode, a windowed plan for
   the diffusion), the precision of a host form, what the plan holds.  These go to the library directly (M.lib()): the
   Python methods catch some of the conditions themselves.

Plans are tiny: ncrms = 11, nx = 4, nz = 6, two tracers, fp64 and fp32, wave-major and reference layout (an odd fp32
plan is wave-major with set_f32_odd_ncrms(1) only).  The block [5, 8): both ends odd, so an fp32 pair is split at either
end and the staged arrays start 4 modulo 8 bytes; and [6, 9), which on the fp64 wave-major plan (8 instances per tile at
nz <= 8) lies across a tile edge.  One windowed plan (nz = 239, ncrms = 3, tall columns on; block [1, 3)) for the calls that
support windows -- all but the diffusion."""
import ctypes
import itertools

import numpy as np
import pytest

import diffuse_model as DM
import subside_model as SM
from plan_harness import _defaults
from util import assert_bitwise, to_dev, to_host

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
T = 2
SEED = 4100

# name -> (shape, dtype, switches, blocks (sl0, n))
KINDS = {
    "f64-wm": ((11, 4, 6), F64, {}, ((5, 3), (6, 3))),
    "f64-ref": ((11, 4, 6), F64, dict(ref=True), ((5, 3), (6, 3))),
    "f32-wm": ((11, 4, 6), F32, dict(odd=True), ((5, 3), (6, 3))),
    "f32-ref": ((11, 4, 6), F32, dict(ref=True), ((5, 3), (6, 3))),
    "f64-tall": ((3, 4, 239), F64, dict(tall=True), ((1, 2),)),
}
SMALL = [k for k in KINDS if "tall" not in k]
CASES = [pytest.param(k, b, id=f"{k}-sl{b[0]}n{b[1]}") for k, v in KINDS.items() for b in v[3]]
CASES_NO_WINDOWS = [c for c in CASES if "tall" not in c.values[0]]


_INPUTS = {}


def inputs(oracle, kind):
    """the seven arrays of KINDS[kind]: computed once and shared; no test writes them"""
    if kind not in _INPUTS:
        shape, dt, _, _ = KINDS[kind]
        _INPUTS[kind] = SM.make_plan_inputs(oracle, shape, T, dt, SEED)
    return _INPUTS[kind]


def new_plan(M, kind, oracle=None):
    """a plan of KINDS[kind] in the layout the kind names (asserted), filled if an oracle is given"""
    shape, dt, sw, _ = KINDS[kind]
    M.set_plan_layout(M.LAYOUT_REFERENCE if sw.get("ref") else M.LAYOUT_WAVEMAJOR)
    M.set_tall_columns(int(bool(sw.get("tall"))))
    M.set_f32_odd_ncrms(int(bool(sw.get("odd"))))
    plan = M.Plan(*shape, T, dtype=dt)
    assert plan.layout == (M.LAYOUT_REFERENCE if sw.get("ref") else M.LAYOUT_WAVEMAJOR), kind
    assert (plan.level_windows > 1) == bool(sw.get("tall")), kind
    if oracle is not None:
        i = inputs(oracle, kind)
        plan.upload(i["f"], i["u"], i["w"], i["rho"], i["rhow"], i["adz"], i["flux"])
    return plan


def state(M, plan):
    """everything the plan holds that a block call may change: f, flux, and u, w through the Courant number"""
    ncrms, nx, nz, nt = plan.dims
    sh = M.host_shapes(ncrms, nx, nz, nt)
    f, flux = np.empty(sh["f"], plan._dt, order="F"), np.empty(sh["flux"], plan._dt, order="F")
    plan.download(f, flux)
    clev, cinst = plan.courant_host()
    return dict(f=f, flux=flux, clev=clev, cinst=cinst)


def same_state(M, a, b, what):
    sa, sb = state(M, a), state(M, b)
    for k in sa:
        assert_bitwise(sa[k], sb[k], f"{what}: {k} of the plan, host form against device form")


def nans(shape, dt):
    return np.full(shape, np.nan, dt, order="F")


def rand(rng, shape, dt, lo=-0.5, hi=0.5):
    return np.asfortranarray(rng.uniform(lo, hi, shape).astype(dt))


def subsets(names, empty=False):
    return [s for r in range(0 if empty else 1, len(names) + 1) for s in itertools.combinations(names, r)]


def dev_or_none(a):
    return None if a is None else to_dev(a)


def test_layouts_covered(mpdata):
    """the kinds are what their names say: both layouts, both precisions, one windowed plan"""
    seen = set()
    for kind in KINDS:
        plan = new_plan(mpdata, kind)
        seen.add((plan.layout, plan._dt, plan.level_windows > 1))
        plan.close()
    W, R = mpdata.LAYOUT_WAVEMAJOR, mpdata.LAYOUT_REFERENCE
    assert seen == {(W, F64, False), (R, F64, False), (W, F32, False), (R, F32, False), (W, F64, True)}


# ---- 1. optional arrays: host form == device form, whatever is absent

@pytest.mark.parametrize("kind,block", CASES)
def test_level_stats_subsets(mpdata, oracle, kind, block):
    (sl0, n), dt, nzm = block, KINDS[kind][1], KINDS[kind][0][2] - 1
    a, b = new_plan(mpdata, kind, oracle), new_plan(mpdata, kind, oracle)
    for sub in subsets(("sum", "min", "max")):
        host = {k: nans((n, nzm, T), dt) for k in sub}
        a.level_stats_host(sl0, n, **host)
        dev = {k: to_dev(nans((n, nzm, T), dt)) for k in sub}
        b.level_stats(sl0, n, **dev)
        b.sync()
        for k in sub:
            assert_bitwise(host[k], to_host(dev[k]), f"level_stats {sub}: {k}")
    a.close()
    b.close()


@pytest.mark.parametrize("kind,block", CASES)
def test_courant_subsets(mpdata, oracle, kind, block):
    """the Python host method always asks for both arrays: the host form is called directly"""
    (sl0, n), dt, nzm = block, KINDS[kind][1], KINDS[kind][0][2] - 1
    a, b = new_plan(mpdata, kind, oracle), new_plan(mpdata, kind, oracle)
    fn = getattr(mpdata.lib(), "mpdata_plan_courant" + a._sfx)
    for sub in subsets(("clev", "cinst")):
        host = {k: nans((n, nzm) if k == "clev" else (n,), dt) for k in sub}
        ptrs = [ctypes.c_void_p(host[k].ctypes.data) if k in sub else None for k in ("clev", "cinst")]
        assert fn(a._p, sl0, n, *ptrs) == 0, mpdata.lib().mpdata_last_error()
        dev = {k: to_dev(host[k] * 0) for k in sub}
        b.courant(sl0, n, **dev)
        b.sync()
        for k in sub:
            assert_bitwise(host[k], to_host(dev[k]), f"courant {sub}: {k}")
    a.close()
    b.close()


@pytest.mark.parametrize("kind,block", CASES)
def test_level_add_modes(mpdata, oracle, kind, block):
    (sl0, n), dt, nzm = block, KINDS[kind][1], KINDS[kind][0][2] - 1
    a, b = new_plan(mpdata, kind, oracle), new_plan(mpdata, kind, oracle)
    rng = np.random.default_rng([SEED, 1, sl0])
    for mode in (mpdata.LEVEL_ADD, mpdata.LEVEL_ADD_CLIP):
        d = rand(rng, (n, nzm, T), dt)
        a.level_add_host(d, sl0, n, mode)
        b.level_add(to_dev(d), sl0, n, mode)
        same_state(mpdata, a, b, f"level_add mode {mode}")
    a.close()
    b.close()


@pytest.mark.parametrize("kind,block", CASES)
def test_scale_uw_subsets(mpdata, oracle, kind, block):
    (sl0, n), dt = block, KINDS[kind][1]
    a, b = new_plan(mpdata, kind, oracle), new_plan(mpdata, kind, oracle)
    rng = np.random.default_rng([SEED, 2, sl0])
    for sub in subsets(("su", "sw")):
        s = {k: rand(rng, (n,), dt, 0.5, 1.5) if k in sub else None for k in ("su", "sw")}
        a.scale_uw_host(s["su"], s["sw"], sl0, n)
        b.scale_uw(dev_or_none(s["su"]), dev_or_none(s["sw"]), sl0, n)
        same_state(mpdata, a, b, f"scale_uw {sub}")
    a.close()
    b.close()


@pytest.mark.parametrize("kind,block", CASES)
def test_column_path_subsets(mpdata, oracle, kind, block):
    (sl0, n), dt, nx = block, KINDS[kind][1], KINDS[kind][0][1]
    a, b = new_plan(mpdata, kind, oracle), new_plan(mpdata, kind, oracle)
    for with_mass in (True, False):
        hp, hm = nans((n, nx, T), dt), nans((n, T), dt) if with_mass else None
        a.column_path_host(hp, hm, sl0, n)
        dp, dm = to_dev(nans((n, nx, T), dt)), to_dev(nans((n, T), dt)) if with_mass else None
        b.column_path(dp, dm, sl0, n)
        b.sync()
        assert_bitwise(hp, to_host(dp), f"column_path, mass {with_mass}: path")
        if with_mass:
            assert_bitwise(hm, to_host(dm), "column_path: mass")
    a.close()
    b.close()


@pytest.mark.parametrize("kind,block", CASES_NO_WINDOWS)
def test_diffuse_subsets(mpdata, oracle, kind, block):
    """sb, st and zflux in all eight combinations: st and zflux move down in the staging buffer when sb is absent"""
    (sl0, n), dt, (_, nx, nz) = block, KINDS[kind][1], KINDS[kind][0]
    a, b = new_plan(mpdata, kind, oracle), new_plan(mpdata, kind, oracle)
    for i, sub in enumerate(subsets(("sb", "st", "zflux"), empty=True)):
        c = DM.make_coeffs(n, nx, nz, dt, SEED + i)
        sb, st = (c[k] if k in sub else None for k in ("sb", "st"))
        hz = nans((n, nz, T), dt) if "zflux" in sub else None
        a.diffuse_host(c["tkh"], c["cx"], c["cz"], sb, st, hz, sl0, n)
        dz = to_dev(nans((n, nz, T), dt)) if "zflux" in sub else None
        b.diffuse(to_dev(c["tkh"]), to_dev(c["cx"]), to_dev(c["cz"]), dev_or_none(sb), dev_or_none(st), dz, sl0, n, ntracers=T)
        same_state(mpdata, a, b, f"diffuse {sub}")
        if "zflux" in sub:
            assert_bitwise(hz, to_host(dz), f"diffuse {sub}: zflux")
    a.close()
    b.close()


@pytest.mark.parametrize("kind,block", CASES)
def test_subside_subsets(mpdata, oracle, kind, block):
    (sl0, n), dt, nzm = block, KINDS[kind][1], KINDS[kind][0][2] - 1
    a, b = new_plan(mpdata, kind, oracle), new_plan(mpdata, kind, oracle)
    rng = np.random.default_rng([SEED, 3, sl0])
    for with_dsum in (True, False):
        cb, cc = rand(rng, (n, nzm), dt, -0.25, 0.25), rand(rng, (n, nzm), dt, -0.25, 0.25)
        hd = nans((n, nzm, T), dt) if with_dsum else None
        a.subside_host(cb, cc, hd, sl0, n)
        dd = to_dev(nans((n, nzm, T), dt)) if with_dsum else None
        b.subside(to_dev(cb), to_dev(cc), dd, sl0, n, ntracers=T)
        same_state(mpdata, a, b, f"subside, dsum {with_dsum}")
        if with_dsum:
            assert_bitwise(hd, to_host(dd), "subside: dsum")
    a.close()
    b.close()


# ---- 2. check order.  name -> (pointer arguments, has a tracer range, has a mode, text of its first own check when every
# pointer is NULL)
CALLS = {
    "level_stats": (3, True, False, "sum, min and max are all NULL"),
    "courant": (2, False, False, "clev and cinst are both NULL"),
    "level_add": (1, True, True, "null d"),
    "scale_uw": (2, False, False, "su and sw are both NULL"),
    "column_path": (2, True, False, "null path"),
    "diffuse": (6, True, False, "null tkh"),
    "subside": (3, True, False, "null cb"),
}
FORMS = ("device", "host")


def raw(M, plan, call, form, sl0, n, ptrs, mode=0, first=0, ntr=1, other_precision=False):
    """one call of the library itself -> (what the call names itself in its texts, return code, error text)"""
    nptr, tracers, has_mode, _ = CALLS[call]
    assert len(ptrs) == nptr
    args = [plan._p, sl0, n, *ptrs] + ([mode] if has_mode else [])
    if form == "device":
        name = f"mpdata_plan_{call}_device"
        args += [first, ntr] if tracers else []
    else:
        f32 = (plan._dt == F32) != other_precision
        name = f"mpdata_plan_{call}" + ("_f32" if f32 else "")
    rc = getattr(M.lib(), name)(*args)
    return name[:-4] if name.endswith("_f32") else name, rc, M.lib().mpdata_last_error().decode()


@pytest.fixture(scope="module")
def somewhere():
    """a valid address for pointer arguments no correct call looks behind: device memory for the device forms, host memory
    for the host forms (1 MiB each: more than any array of these plans)"""
    import torch
    dev, host = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda:0"), np.zeros(1 << 20, np.uint8)
    yield {"device": ctypes.c_void_p(dev.data_ptr()), "host": ctypes.c_void_p(host.ctypes.data)}


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("kind", SMALL)
def test_check_order(mpdata, oracle, somewhere, kind, call, form):
    M = mpdata
    nptr, tracers, has_mode, null_text = CALLS[call]
    ncrms = KINDS[kind][0][0]
    none, valid = [None] * nptr, [somewhere[form]] * nptr
    plan, fresh = new_plan(M, kind, oracle), new_plan(M, kind)
    # the block before the NULLs
    what, rc, text = raw(M, plan, call, form, ncrms - 2, 3, none)
    assert rc == M.EINVAL and text.startswith(f"{what}: instances [{ncrms - 2}, {ncrms + 1}) outside"), text
    # the tracer range before the NULLs
    if tracers and form == "device":
        what, rc, text = raw(M, plan, call, form, 5, 3, none, first=T, ntr=1)
        assert rc == M.EINVAL and text.startswith(f"tracer range [{T}, {T + 1}) outside"), text
    # the call's own arguments before what the plan holds ...
    what, rc, text = raw(M, fresh, call, form, 5, 3, none)
    assert rc == M.EINVAL and text == f"{what}: {null_text}", text
    if has_mode:
        what, rc, text = raw(M, fresh, call, form, 5, 3, valid, mode=7)
        assert rc == M.EINVAL and text == f"{what}: unknown mode 7", text
    if form == "host":
        # ... and before the precision
        what, rc, text = raw(M, plan, call, form, 5, 3, none, other_precision=True)
        assert rc == M.EINVAL and text == f"{what}: {null_text}", text
        if has_mode:
            what, rc, text = raw(M, plan, call, form, 5, 3, valid, mode=7, other_precision=True)
            assert rc == M.EINVAL and text == f"{what}: unknown mode 7", text
        # the precision before what the plan holds
        what, rc, text = raw(M, fresh, call, form, 5, 3, valid, other_precision=True)
        assert rc == M.ESTATE and text.startswith("plan precision ("), text
    # and last what the plan holds
    what, rc, text = raw(M, fresh, call, form, 5, 3, valid)
    assert rc == M.ESTATE and text == f"{what} before upload / import", text
    plan.close()
    fresh.close()


@pytest.mark.parametrize("form", FORMS)
def test_diffuse_windowed_check_order(mpdata, somewhere, form):
    """a windowed plan refuses the diffusion after the NULLs and before the precision and the state"""
    M = mpdata
    plan = new_plan(M, "f64-tall")   # (never filled: the refusal comes first)
    valid = [somewhere[form]] * 6
    what, rc, text = raw(M, plan, "diffuse", form, 1, 2, [None] + valid[1:])
    assert rc == M.EINVAL and text == f"{what}: null tkh", text
    what, rc, text = raw(M, plan, "diffuse", form, 1, 2, valid, other_precision=True)
    assert rc == M.EUNSUPPORTED and text.startswith(f"{what} on a windowed plan"), text
    plan.close()
