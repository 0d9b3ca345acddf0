"""CPU tests of the per-level increments (include/mpdata_hip.h 3i): the model against an explicit loop, the guard on the
seeded inputs of the GPU tests, the plan model's new call, the declarations of the five entry points in the header, the
Python binding and the Fortran interface, and the argument errors that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest

import level_add_model as AM
import level_stats_model as LM
from oracle import plan_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mpdata_plan_level_add_device", "mpdata_plan_level_add", "mpdata_plan_level_add_f32",
         "mpdata_level_add_device", "mpdata_level_add_f32_device")


# ---- the model is right
@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("clip", [False, True])
def test_model_equals_a_triple_loop(dt, clip):
    rng = np.random.default_rng(7)
    f = np.asfortranarray(rng.uniform(-1, 1, (3, 2 + 6, 4, 2)).astype(dt))
    d = np.asfortranarray(rng.uniform(-1, 1, (3, 4, 2)).astype(dt))
    want = np.empty_like(f)
    for sl in range(3):
        for i in range(8):
            for k in range(4):
                for t in range(2):
                    x = dt(f[sl, i, k, t] + d[sl, k, t])
                    want[sl, i, k, t] = max(dt(0), x) if clip else x
    got = AM.level_add(f, d, clip)
    assert got.dtype == dt and got.flags["F_CONTIGUOUS"]
    assert np.array_equal(LM.bits(got), LM.bits(want))
    assert bool(np.any(got != f + d[:, None])) == clip          # (CLIP bites here)
    one = AM.level_add(f[..., 0], d[..., 0], clip)                # no tracer axis
    assert np.array_equal(LM.bits(one), LM.bits(want[..., 0]))


def test_add_keeps_the_sign_of_a_zero_sum():
    f = np.array([[[0.0], [-0.0], [1.5], [-0.0], [0.0], [-0.0], [-0.0]]], order="F")     # (1, 7, 1)
    assert np.signbit(AM.level_add(f, np.array([[-0.0]]))[0, :, 0]).tolist() == [False, True, False, True, False, True, True]
    assert not np.signbit(AM.level_add(f, np.array([[-1.5]]))[0, 2, 0])                 # 1.5 - 1.5 = +0 (round to nearest)
    assert not AM.canon(np.array([-0.0, 0.0, -1.0])).view(np.uint64)[:2].any()


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_two_adds_are_two_roundings(dt):
    shape = (5, 7, 12)
    rng = np.random.default_rng(11)
    f = np.asfortranarray(rng.uniform(0, 1, (5, 13, 11)).astype(dt))
    d1, d2 = AM.make_d(shape, 1, dt, 1), AM.make_d(shape, 1, dt, 2)
    two = AM.level_add(AM.level_add(f, d1), d2)
    once = AM.level_add(f, d1 + d2)
    assert np.array_equal(two, (f + d1[:, None]) + d2[:, None])
    assert np.any(LM.bits(two) != LM.bits(once))


# ---- the inputs are sharp
@pytest.mark.parametrize("name", list(LM.INPUTS))
def test_inputs_are_sharp(oracle, name):
    """f of LM.INPUTS[name] with the first d the GPU tests add to it: the add is inexact on at least a quarter of the
    cells, CLIP changes between 5 % and 95 % of them, and no sum is zero (the sign of a clipped zero is unspecified)"""
    shape, T, dt, seed = LM.INPUTS[name]
    f = LM.make(oracle, shape, T, dt, seed)["f"]
    d = AM.first_d(name)
    assert d.dtype == dt and d.shape == f.shape[:1] + f.shape[2:] and d.flags["F_CONTIGUOUS"]
    assert np.any(d > 0) and np.any(d < 0) and np.all(np.isfinite(d))
    s = AM.level_add(f, d)
    inexact = float(np.mean((s - f) != d[:, None]))
    clipped = float(np.mean(LM.bits(AM.level_add(f, d, True)) != LM.bits(s)))
    print(f"{name}: inexact on {inexact:.2f}, CLIP changes {clipped:.2f} of {s.size} cells")
    assert inexact >= 0.25, (name, inexact)
    assert 0.05 <= clipped <= 0.95, (name, clipped)
    assert not np.any(s == 0), name
    for sl0, n in ((0, 1), (10, 1), (3, 5), (1, 9)):     # the blocks of the GPU tests are slices of the same d
        if sl0 + n <= shape[0]:
            assert np.array_equal(AM.level_add(f[sl0:sl0 + n], d[sl0:sl0 + n]), s[sl0:sl0 + n])


# ---- PlanModelAdd.level_add
def _model(oracle, name, boundary):
    shape, T, dt, seed = LM.INPUTS[name]
    m = AM.PlanModelAdd(oracle, *shape, T, dt)
    inp = LM.make(oracle, shape, T, dt, seed)
    return m, inp


def _same(a, b):
    for k in PM.NAMES:
        assert np.array_equal(LM.bits(a.a[k]), LM.bits(b.a[k])), k
    assert (a.boundary, a.uploaded, a.have_u, a.have_w, a.timing, a.ran, a.steps) == (b.boundary, b.uploaded, b.have_u, b.have_w,
                                                                                 b.timing, b.ran, b.steps)


def test_plan_model_add_errors_leave_the_model_unchanged(oracle):
    name = "f64-blocks"
    shape, T, dt, seed = LM.INPUTS[name]
    ncrms, nzm = shape[0], shape[2] - 1
    m, inp = _model(oracle, name, PM.GIVEN)
    d = AM.first_d(name)
    assert m.level_add(d) == PM.ESTATE                       # never filled
    assert m.upload(inp) is None
    keep, _ = _model(oracle, name, PM.GIVEN)
    assert keep.upload(inp) is None
    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, ncrms + 1), (ncrms, 1), (5, 7)):
        assert m.level_add(d[:max(n, 1)], sl0, n) == PM.EINVAL, (sl0, n)
    assert m.level_add(None) == PM.EINVAL
    assert m.level_add(d, mode=2) == PM.EINVAL and m.level_add(d, mode=-1) == PM.EINVAL
    assert m.level_add(d, first=1) == PM.EINVAL              # three tracers from tracer 1
    assert m.level_add(d[..., 0], first=T) == PM.EINVAL and m.level_add(d[..., 0], first=-1) == PM.EINVAL
    m.multi = True
    assert m.level_add(d) == PM.EUNSUPPORTED and m.level_add(d, 0, 0) == PM.EINVAL
    m.multi = False
    _same(m, keep)
    assert m.level_add(d) is None and not np.array_equal(m.a["f"], keep.a["f"])


@pytest.mark.parametrize("boundary", [PM.GIVEN, PM.PERIODIC])
@pytest.mark.parametrize("mode", [AM.ADD, AM.CLIP])
def test_plan_model_add_is_export_change_import(oracle, boundary, mode):
    name = "f64-blocks"
    shape, T, dt, seed = LM.INPUTS[name]
    a, inp = _model(oracle, name, boundary)
    b, _ = _model(oracle, name, boundary)
    d = AM.first_d(name)
    for m in (a, b):
        assert m.upload(inp) is None and m.set_boundary(boundary) is None and m.run() is None     # (halos stale)
    assert a.level_add(d, mode=mode) is None
    exp = b.export_device(("f",))["f"]
    assert b.import_device({"f": AM.level_add(exp, d, mode == AM.CLIP)}) is None
    for m in (a, b):
        assert m.run(1, 2) is None
    ea, eb = a.export_device(), b.export_device()
    for k in ea:
        assert np.array_equal(LM.bits(ea[k]), LM.bits(eb[k])), k
    # a block and a tracer range: the same through the block calls
    blk = np.asfortranarray(d[3:8, :, 1:3])
    assert a.level_add(blk, 3, 5, mode, 1) is None
    exp = b.export_block(3, 5, ("f",), 1, 2)["f"]
    assert b.import_block(3, 5, {"f": AM.level_add(exp, blk, mode == AM.CLIP)}, 1, 2) is None
    assert a.set_boundary(PM.GIVEN) is None and b.set_boundary(PM.GIVEN) is None
    _same(a, b)


# ---- the bindings exist (files parsed: no device, no library)
def test_header_python_and_fortran_name_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "mpdata_hip.h")).read()
    capi = open(os.path.join(ROOT, "codesign-kernels_amd", "capi.py")).read()
    f90 = open(os.path.join(ROOT, "codesign-kernels_amd", "fortran", "mpdata_hip_mod.F90")).read()
    assert "---- 3i." in hdr
    assert re.search(r"#define\s+MPDATA_LEVEL_ADD\s+0\b", hdr) and re.search(r"#define\s+MPDATA_LEVEL_ADD_CLIP\s+1\b", hdr)
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", hdr), f"header: {n}"
        assert re.search(r"\b" + n + r"\b", capi), f"capi.py: {n}"
        assert re.search(r'"' + n + r'"', f90), f"Fortran interface: {n}"
    for n in ("mpdata_plan_level_add_device_c", "mpdata_plan_level_add_c", "mpdata_level_add_device_c"):
        assert re.search(r"integer\(c_int\) function " + n + r"\(", f90), n
        assert re.search(r"public ::.*\b" + n + r"\b", f90), n
    assert re.search(r"^LEVEL_ADD, LEVEL_ADD_CLIP = 0, 1\b", capi, re.M)
    for n in ("def level_add(self, d,", "def level_add_host(self, d,", "def level_add(f, d,"):
        assert n in capi, n
    init = open(os.path.join(ROOT, "codesign-kernels_amd", "__init__.py")).read()
    for n in ("level_add", "LEVEL_ADD", "LEVEL_ADD_CLIP"):
        assert f'"{n}"' in init, n


def test_argument_errors_without_device(mpdata):
    L = mpdata.lib()
    one = ctypes.c_void_p(8)   # never dereferenced: the checks come before anything looks at the arrays
    assert (mpdata.LEVEL_ADD, mpdata.LEVEL_ADD_CLIP) == (0, 1)
    for fn in (L.mpdata_level_add_device, L.mpdata_level_add_f32_device):
        assert fn(4, 5, 6, 1, None, one, 0, None) == mpdata.EINVAL          # null f
        assert b"null f" in L.mpdata_last_error()
        assert fn(4, 5, 6, 1, one, None, 0, None) == mpdata.EINVAL          # null d
        assert b"null d" in L.mpdata_last_error()
        assert fn(4, 0, 6, 1, one, one, 0, None) == mpdata.EINVAL           # nx < 1
        assert fn(4, 5, 1, 1, one, one, 0, None) == mpdata.EINVAL           # nz < 2
        assert b"nz=1" in L.mpdata_last_error()
        assert fn(0, 5, 6, 1, one, one, 0, None) == mpdata.EINVAL
        assert fn(4, 5, 6, 0, one, one, 0, None) == mpdata.EINVAL
        assert fn(4, 5, 6, 1, one, one, 2, None) == mpdata.EINVAL           # unknown mode
        assert fn(4, 5, 6, 1, one, one, -1, None) == mpdata.EINVAL
        assert b"unknown mode" in L.mpdata_last_error()
    assert L.mpdata_plan_level_add_device(None, 0, 1, one, 0, 0, 1) == mpdata.EINVAL
    assert L.mpdata_plan_level_add(None, 0, 1, one, 0) == mpdata.EINVAL
    assert L.mpdata_plan_level_add_f32(None, 0, 1, one, 0) == mpdata.EINVAL
    for n, sl0 in ((0, 0), (-2, 0), (1, -1)):   # (checked before the plan is looked at)
        assert L.mpdata_plan_level_add_device(one, sl0, n, one, 0, 0, 1) == mpdata.EINVAL


def test_new_kernels_do_not_spill():
    """the resource-usage report the build writes next to the object of mpdata_level_add.hip"""
    rep = os.path.join(ROOT, "codesign-kernels_amd", "csrc", "mpdata_level_add.usage.txt")
    if not os.path.exists(rep):
        pytest.skip("no resource-usage report (library not built here)")
    txt = open(rep).read()
    assert len(re.findall(r"Function Name: \S*level_add_kernel", txt)) == 4
    assert [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", txt)] == [0, 0, 0, 0]
    assert {int(x) for x in re.findall(r"VGPRs Spill: (\d+)", txt)} == {0}
    assert re.search(r"LDS Size \[bytes/block\]: [1-9]", txt) is None
