"""CPU tests of the large-scale vertical advection (include/mpdata_hip.h 3m): the numpy model of tests/subside_model.py
against what the definition implies -- the merge property of level windows, a field constant in k, SAM's if / else form --,
the plan model's rules, and the interface (header, ctypes, Fortran, Python names, the argument checks that need no
device, the compiler's resource report).  No test here needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import subside_model as SM
from oracle import plan_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mpdata_plan_subside_device", "mpdata_plan_subside", "mpdata_plan_subside_f32", "mpdata_subside_device",
         "mpdata_subside_f32_device")
DTYPES = [np.float64, np.float32]


def field(n, nx, nz, T, dtype, seed):
    rng = np.random.default_rng([seed, n, nx, nz, T])
    sh = (n, nx + 6, nz - 1) + ((T,) if T > 1 else ())
    return np.asfortranarray(rng.uniform(-1.0, 1.0, sh).astype(dtype))


# ---- the model against the definition's consequences
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("nz", [239, 250, 300, 1000])
def test_windows_merge_to_the_tall_operator(mpdata, nz, dtype):
    """the operator on every level window as a problem of its own (clamped at the window's edges, the coefficients of the
    tall levels it stands for), owned levels merged == the operator on the tall column, bit for bit; the geometry is the
    library's.  A margin of 3 levels exceeds the radius of 1."""
    n, nx, T = 2, 3, 2
    nzm = nz - 1
    f = field(n, nx, nz, T, dtype, 21)
    cb, cc = SM.make_coeffs(n, nz, dtype, 22)
    want, want_d = SM.subside(f, cb, cc)
    W = mpdata.level_window(nz, 0)[0]
    assert W > 1
    got, got_d = np.full_like(want, np.nan), np.full_like(want_d, np.nan)
    owned = np.zeros(nzm, int)
    for h in range(W):
        _, k0, nz_w, own0, own1 = mpdata.level_window(nz, h)
        lev = slice(k0, k0 + nz_w - 1)
        new, d = SM.subside(np.asfortranarray(f[:, :, lev]), np.asfortranarray(cb[:, lev]), np.asfortranarray(cc[:, lev]))
        assert k0 + 1 <= own0 <= own1 <= k0 + nz_w - 1
        own = slice(own0 - 1, own1)                      # tall, 0-based
        loc = slice(own0 - 1 - k0, own1 - k0)            # in the window
        got[:, :, own], got_d[:, own] = new[:, :, loc], d[:, loc]
        owned[own] += 1
    assert np.all(owned == 1)                            # every tall level owned exactly once
    assert np.array_equal(SM.bits(got), SM.bits(want)) and np.array_equal(SM.bits(got_d), SM.bits(want_d))
    assert not np.array_equal(want, f)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_a_field_constant_in_k_keeps_every_bit(dtype):
    """for any cb, cc of either sign, on inputs without -0.0 (a -0.0 may come back as +0.0 through -0 - (-0))"""
    n, nx, nz = 3, 4, 9
    rng = np.random.default_rng(5)
    col = rng.uniform(-2.0, 2.0, (n, nx + 6, 1)).astype(dtype)
    col[0, 1, 0] = 0.0
    f = np.asfortranarray(np.repeat(col, nz - 1, axis=2))
    assert not np.any(np.signbit(f) & (f == 0))
    cb, cc = SM.make_coeffs(n, nz, dtype, 6)
    assert (cb < 0).any() and (cb > 0).any() and (cc < 0).any() and (cc > 0).any()
    new, dsum = SM.subside(f, cb, cc)
    assert np.array_equal(SM.bits(new), SM.bits(f))
    assert not np.any(dsum)
    # ... and the stated exception: -0.0 with two negative coefficients
    z = np.full((1, 7, 3), -0.0, dtype, order="F")
    neg = np.full((1, 3), -0.25, dtype, order="F")
    new, _ = SM.subside(z, neg, neg)
    assert not np.any(new) and not np.any(np.signbit(new))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_sams_folding_is_the_if_else_form(dtype):
    """one of cb, cc zero per level, both zero at k = 1 and k = nzm: the result equals upwind differencing written with an
    if on the sign of the velocity, on inputs without zeros"""
    n, nx, nz = 4, 5, 12
    nzm = nz - 1
    f = field(n, nx, nz, 1, dtype, 31)
    assert not np.any(f == 0)
    rng = np.random.default_rng(32)
    wsub = rng.uniform(-0.4, 0.4, (n, nzm)).astype(dtype)
    wsub[:, 0] = 0
    wsub[:, -1] = 0
    up = wsub >= 0
    cb = np.asfortranarray(np.where(up, wsub, 0).astype(dtype))
    cc = np.asfortranarray(np.where(up, 0, wsub).astype(dtype))
    new, dsum = SM.subside(f, cb, cc)
    want = np.array(f, order="F")
    for k in range(nzm):
        for b in range(n):
            if wsub[b, k] >= 0:
                d = wsub[b, k] * (f[b, :, k] - f[b, :, max(k - 1, 0)])
            else:
                d = wsub[b, k] * (f[b, :, min(k + 1, nzm - 1)] - f[b, :, k])
            assert d.dtype == dtype
            want[b, :, k] = f[b, :, k] - d
    assert np.array_equal(SM.bits(new), SM.bits(want))
    assert np.array_equal(SM.bits(new[:, :, [0, nzm - 1]]), SM.bits(f[:, :, [0, nzm - 1]]))      # the end levels do not move
    assert not np.array_equal(new, f)


def test_one_tracer_with_and_without_axis_and_dsum_is_the_interior_sum():
    n, nx, nz = 3, 3, 6
    f = field(n, nx, nz, 2, np.float64, 14)
    cb, cc = SM.make_coeffs(n, nz, np.float64, 5)
    new, ds = SM.subside(f, cb, cc)
    for t in range(2):
        n1, d1 = SM.subside(np.asfortranarray(f[..., t]), cb, cc)
        assert np.array_equal(SM.bits(n1), SM.bits(new[..., t])) and np.array_equal(SM.bits(d1), SM.bits(ds[..., t]))
    dec = f - new
    assert np.allclose(ds, dec[:, 3:nx + 3].sum(axis=1), rtol=0, atol=1e-14)
    assert not np.array_equal(new[:, :3], f[:, :3]) and not np.array_equal(new[:, nx + 3:], f[:, nx + 3:])   # halos move too


# ---- the plan model: order of the checks, the block and the wrap rule
def _model(oracle, dtype=np.float64, T=2, shape=(5, 8, 6)):
    m = SM.PlanModelSubside(oracle, *shape, T, dtype)
    return m, SM.make_plan_inputs(oracle, shape, T, dtype, 100)


def test_plan_model_errors_change_nothing(oracle):
    m, inp = _model(oracle)
    cb, cc = SM.make_coeffs(5, 6, np.float64, 6)
    assert m.subside(cb, cc) == PM.ESTATE                                  # never filled
    assert m.upload(inp) is None
    keep = {k: np.array(v) for k, v in m.a.items()}
    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, 6), (5, 1), (3, 3)):
        assert m.subside(cb, cc, sl0=sl0, n=n) == PM.EINVAL, (sl0, n)
    assert m.subside(cb, cc, first=1, ntr=2) == PM.EINVAL and m.subside(cb, cc, first=-1, ntr=1) == PM.EINVAL
    assert m.subside(cb, cc, first=0, ntr=0) == PM.EINVAL
    assert m.subside(None, cc) == PM.EINVAL and m.subside(cb, None) == PM.EINVAL
    assert m.subside(cb, cc, eb=4) == PM.ESTATE                            # a host form of the other precision
    assert m.subside(None, cc, eb=4) == PM.EINVAL                          # the NULLs come first
    m.multi = True
    assert m.subside(cb, cc) == PM.EUNSUPPORTED and m.subside(cb, cc, sl0=0, n=0) == PM.EINVAL
    m.multi = False
    for k, v in keep.items():
        assert np.array_equal(SM.bits(m.a[k]), SM.bits(v)), k
    d = m.subside(cb, cc)
    assert d.shape == (5, 5, 2) and not np.array_equal(m.a["f"], keep["f"])
    for k in ("u", "w", "rho", "rhow", "adz", "flux"):
        assert np.array_equal(SM.bits(m.a[k]), SM.bits(keep[k])), k


@pytest.mark.parametrize("boundary", [PM.GIVEN, PM.PERIODIC])
def test_plan_model_subside_is_export_change_import(oracle, boundary):
    """the call on a block and a tracer = export of the block, the operator, import -- also on a PERIODIC model with stale
    halos: no wrap is part of the call, and none is needed"""
    a, inp = _model(oracle)
    b, _ = _model(oracle)
    for m in (a, b):
        assert m.upload(inp) is None and m.set_boundary(boundary) is None and m.run() is None     # (halos stale)
    cb, cc = SM.make_coeffs(3, 6, np.float64, 7)
    d = a.subside(cb, cc, sl0=1, n=3, first=1, ntr=1)
    exp = b.export_block(1, 3, ("f",), 1, 1)["f"]
    new, d2 = SM.subside(exp[..., 0], cb, cc)
    assert b.import_block(1, 3, {"f": new}, 1, 1) is None
    assert np.array_equal(SM.bits(d[..., 0]), SM.bits(d2))
    for m in (a, b):
        assert m.run() is None
    ea, eb = a.export_device(), b.export_device()
    for k in ea:
        assert np.array_equal(SM.bits(ea[k]), SM.bits(eb[k])), k


# ---- the interface (files parsed: no device)
def test_python_names(mpdata):
    assert callable(mpdata.subside_device) and callable(mpdata.Plan.subside) and callable(mpdata.Plan.subside_host)
    assert "subside_device" in mpdata.__all__


def _c_params(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"header: {name}"
    return [p.strip() for p in m.group(1).split(",")]


def test_header_ctypes_and_fortran_agree(mpdata):
    hdr = open(os.path.join(ROOT, "include", "mpdata_hip.h")).read()
    f90 = open(os.path.join(ROOT, "codesign-kernels_amd", "fortran", "mpdata_hip_mod.F90")).read()
    sec = hdr.split("---- 3m.")[1].split("---- 4.")[0]
    assert "-0.0" in sec and "windowed plans" in sec.lower() and "are supported" in sec
    L = mpdata.lib()
    ckind = {ctypes.c_int64: "int64_t", ctypes.c_int: "int", ctypes.c_void_p: "*"}
    for n in NAMES:
        params = _c_params(hdr, n)
        fn = getattr(L, n)                                   # the library exports it
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(params), n
        for a, p in zip(fn.argtypes, params):
            k = ckind[a]
            assert ("*" in p) if k == "*" else (p.startswith(k + " ") and "*" not in p), (n, p, a)
    # Fortran: the one interface, bound by the literal name, public, the dummy arguments in the header's order
    m = re.search(r"integer\(c_int\) function mpdata_plan_subside_device_c\(([^)]*)\)\s*&?\s*bind\(C, name=\"mpdata_plan_subside_device\"\)", f90)
    assert m
    fargs = [a.strip() for a in m.group(1).replace("&", " ").split(",")]
    cargs = [re.split(r"[\s*]+", p)[-1] for p in _c_params(hdr, "mpdata_plan_subside_device")]
    assert fargs == cargs, (fargs, cargs)
    assert re.search(r"public ::.*\bmpdata_plan_subside_device_c\b", f90)
    assert "MPDATA_C_PLAN_SUBSIDE" not in f90 and "MPDATA_C_SUBSIDE" not in f90        # no per-precision macro


def test_argument_errors_without_device(mpdata):
    L = mpdata.lib()
    one = ctypes.c_void_p(8)   # never dereferenced: the checks come before anything looks at the arrays
    for fn in (L.mpdata_subside_device, L.mpdata_subside_f32_device):
        assert fn(4, 0, 6, 1, one, one, one, None, None) == mpdata.EINVAL           # nx < 1
        assert fn(4, 5, 1, 1, one, one, one, None, None) == mpdata.EINVAL           # nz < 2
        assert b"nz=1" in L.mpdata_last_error()
        assert fn(0, 5, 6, 1, one, one, one, None, None) == mpdata.EINVAL
        assert fn(4, 5, 6, 0, one, one, one, None, None) == mpdata.EINVAL
        for i, nm in enumerate(("f", "cb", "cc")):
            args = [one, one, one]
            args[i] = None
            assert fn(4, 5, 6, 1, *args, None, None) == mpdata.EINVAL, nm
            assert b"null " + nm.encode() in L.mpdata_last_error()
        assert fn(4, 5, 1, 1, None, None, None, None, None) == mpdata.EINVAL and b"nz=1" in L.mpdata_last_error()   # sizes first
        assert fn(4, 5, 6, 1, None, None, one, None, None) == mpdata.EINVAL and b"null f" in L.mpdata_last_error()  # then f
    assert L.mpdata_plan_subside_device(None, 0, 1, one, one, None, 0, 1) == mpdata.EINVAL
    assert b"null plan" in L.mpdata_last_error()
    assert L.mpdata_plan_subside(None, 0, 1, one, one, None) == mpdata.EINVAL
    assert L.mpdata_plan_subside_f32(None, 0, 1, one, one, None) == mpdata.EINVAL
    for n, sl0 in ((0, 0), (-2, 0), (1, -1)):   # (checked before the plan is looked at)
        assert L.mpdata_plan_subside_device(one, sl0, n, one, one, None, 0, 1) == mpdata.EINVAL
    assert L.mpdata_plan_subside_device(one, 0, 0, None, None, None, 0, 1) == mpdata.EINVAL
    assert b"null c" not in L.mpdata_last_error()                                   # the range came first


def test_new_kernels_do_not_spill():
    """the resource-usage report the build writes next to the object of mpdata_subside.hip"""
    rep = os.path.join(ROOT, "codesign-kernels_amd", "csrc", "mpdata_subside.usage.txt")
    if not os.path.exists(rep):
        pytest.skip("no resource-usage report (library not built here)")
    txt = open(rep).read()
    assert len(re.findall(r"Function Name: \S*wm_subside_kernel", txt)) == 2
    assert len(re.findall(r"Function Name: \S*ref_subside_kernel", txt)) == 2
    assert len(re.findall(r"Function Name: \S*ref_subside_store_kernel", txt)) == 2
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", txt)]
    assert scratch and set(scratch) == {0}
    assert {int(x) for x in re.findall(r"VGPRs Spill: (\d+)", txt)} == {0}
    assert {int(x) for x in re.findall(r"SGPRs Spill: (\d+)", txt)} == {0}
