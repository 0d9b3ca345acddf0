"""CPU tests of the sedimentation (include/mpdata_hip.h 3n): the numpy model of tests/sediment_model.py against a scalar
triple loop and against what the definition implies -- wp = 0, a single non-zero cell, the merge property of level
windows --, the plan model's rules, and the interface (header, ctypes, Fortran, Python names, the argument checks that
need no device, the compiler's resource report).  No test here needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import sediment_model as SM
from oracle import plan_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mpdata_plan_sediment_device", "mpdata_plan_sediment", "mpdata_plan_sediment_f32", "mpdata_sediment_device",
         "mpdata_sediment_f32_device")
DTYPES = [np.float64, np.float32]


def field(n, nx, nz, T, dtype, seed):
    rng = np.random.default_rng([seed, n, nx, nz, T])
    sh = (n, nx + 6, nz - 1) + ((T,) if T > 1 else ())
    return np.asfortranarray(rng.uniform(-1.0, 1.0, sh).astype(dtype))


def coeffs(n, nz, dtype, seed):
    rng = np.random.default_rng([seed, n, nz])
    return tuple(np.asfortranarray(rng.uniform(0.5, 1.0, (n, nz - 1)).astype(dtype)) for _ in range(2))


# ---- the model against the definition
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_model_is_the_scalar_triple_loop(dtype):
    n, nx, nz, T = 3, 4, 6, 2
    nzm = nz - 1
    R = np.dtype(dtype).type
    f = field(n, nx, nz, T, dtype, 11)
    rho, adz = coeffs(n, nz, dtype, 12)
    wp = SM.make_wp(n, nx, nz, T, dtype, 13)
    assert (wp < 0).any() and (wp > 0).any()
    new, psfc, pflux = SM.sediment(f, rho, adz, wp)
    want, ws, wf = np.array(f, order="F"), np.zeros((n, nx, T), dtype), np.zeros((n, nzm, T), dtype)
    for t in range(T):
        for b in range(n):
            for k in range(nzm):
                ir = R(R(1) / R(rho[b, k] * adz[b, k]))
                s = R(0)
                for i in range(nx):
                    fz = R(wp[b, i, k, t] * f[b, i + 3, k, t])
                    fzu = R(wp[b, i, k + 1, t] * f[b, i + 3, k + 1, t]) if k + 1 < nzm else R(0)
                    want[b, i + 3, k, t] = R(f[b, i + 3, k, t] - R(R(fz - fzu) * ir))
                    s = R(s + fz)
                    if k == 0:
                        ws[b, i, t] = fz
                wf[b, k, t] = s
    assert np.array_equal(SM.bits(new), SM.bits(want))
    assert np.array_equal(SM.bits(psfc), SM.bits(ws)) and np.array_equal(SM.bits(pflux), SM.bits(wf))
    assert not np.array_equal(new, f)
    # one tracer with and without the axis
    n1, s1, p1 = SM.sediment(np.asfortranarray(f[..., 1]), rho, adz, np.asfortranarray(wp[..., 1]))
    assert np.array_equal(SM.bits(n1), SM.bits(new[..., 1])) and np.array_equal(SM.bits(s1), SM.bits(psfc[..., 1]))
    assert np.array_equal(SM.bits(p1), SM.bits(pflux[..., 1]))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_wp_zero_keeps_every_bit(dtype):
    """on inputs without -0.0 (a -0.0 may come back as +0.0); psfc = pflux = 0"""
    n, nx, nz = 3, 4, 9
    f = field(n, nx, nz, 1, dtype, 5)
    f[0, 4, 2] = 0.0
    assert not np.any(np.signbit(f) & (f == 0))
    rho, adz = coeffs(n, nz, dtype, 6)
    new, psfc, pflux = SM.sediment(f, rho, adz, np.zeros((n, nx, nz - 1), dtype, order="F"))
    assert np.array_equal(SM.bits(new), SM.bits(f))
    assert not np.any(psfc) and not np.any(pflux)
    # ... and the stated exception: at the top level Fz(k+1) is +0, so -0 - (-0 - +0) * ir = -0 - (-0) = +0
    z = np.full((1, 7, 3), -0.0, dtype, order="F")
    new, _, _ = SM.sediment(z, rho[:1, :3], adz[:1, :3], np.zeros((1, 1, 3), dtype, order="F"))
    assert not np.any(new) and np.signbit(new[0, 3]).tolist() == [True, True, False]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_a_single_cell_moves_mass_one_level_down(dtype):
    """rho = adz = 1, wp = 1/4 everywhere: the cell loses a quarter, the cell below gains it, nothing else moves; from
    level 1 the quarter leaves through the surface"""
    n, nx, nz = 1, 3, 7
    one = np.ones((n, nz - 1), dtype, order="F")
    wp = np.full((n, nx, nz - 1), 0.25, dtype, order="F")
    f = np.zeros((n, nx + 6, nz - 1), dtype, order="F")
    f[0, 4, 3] = 8.0
    new, psfc, pflux = SM.sediment(f, one, one, wp)
    want = np.array(f)
    want[0, 4, 3], want[0, 4, 2] = 6.0, 2.0
    assert np.array_equal(new, want) and not np.any(psfc)
    assert pflux[0, 3] == 2.0 and np.count_nonzero(pflux) == 1
    f = np.zeros_like(f)
    f[0, 3, 0] = 8.0
    new, psfc, pflux = SM.sediment(f, one, one, wp)
    assert new[0, 3, 0] == 6.0 and np.count_nonzero(new) == 1 and psfc[0, 0] == 2.0 and np.count_nonzero(psfc) == 1


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("nz", [239, 250, 300, 1000])
def test_windows_merge_to_the_tall_operator(mpdata, nz, dtype):
    """the operator on every level window as a problem of its own (nothing entering through the window's top, wp and ir
    of the tall levels it stands for), owned levels merged == the operator on the tall column, bit for bit; psfc from the
    owner of level 1, pflux from each level's owner.  The geometry is the library's.  A margin of 3 levels exceeds the
    reach of 1."""
    n, nx, T = 2, 3, 2
    nzm = nz - 1
    f = field(n, nx, nz, T, dtype, 21)
    rho, adz = coeffs(n, nz, dtype, 22)
    wp = SM.make_wp(n, nx, nz, T, dtype, 23)
    want, want_s, want_p = SM.sediment(f, rho, adz, wp)
    W = mpdata.level_window(nz, 0)[0]
    assert W > 1
    got, got_p, got_s = np.full_like(want, np.nan), np.full_like(want_p, np.nan), None
    got[:, :3], got[:, nx + 3:] = f[:, :3], f[:, nx + 3:]
    owned = np.zeros(nzm, int)
    for h in range(W):
        _, k0, nz_w, own0, own1 = mpdata.level_window(nz, h)
        lev = slice(k0, k0 + nz_w - 1)
        new, s, p = SM.sediment(np.asfortranarray(f[:, :, lev]), np.asfortranarray(rho[:, lev]), np.asfortranarray(adz[:, lev]),
                                np.asfortranarray(wp[:, :, lev]))
        assert k0 + 1 <= own0 <= own1 <= k0 + nz_w - 1
        own = slice(own0 - 1, own1)                      # tall, 0-based
        loc = slice(own0 - 1 - k0, own1 - k0)            # in the window
        got[:, 3:nx + 3, own], got_p[:, own] = new[:, 3:nx + 3, loc], p[:, loc]
        if own0 == 1:
            got_s = s
        owned[own] += 1
    assert np.all(owned == 1)                            # every tall level owned exactly once
    assert np.array_equal(SM.bits(got), SM.bits(want)) and np.array_equal(SM.bits(got_p), SM.bits(want_p))
    assert np.array_equal(SM.bits(got_s), SM.bits(want_s))
    assert not np.array_equal(want, f)


# ---- the plan model: order of the checks, the block, the interior-only and the periodic rule
def _model(oracle, dtype=np.float64, T=2, shape=(5, 8, 6)):
    m = SM.PlanModelSediment(oracle, *shape, T, dtype)
    return m, SM.make_plan_inputs(oracle, shape, T, dtype, 100)


def test_plan_model_errors_change_nothing(oracle):
    m, inp = _model(oracle)
    wp = SM.make_wp(5, 8, 6, 2, np.float64, 6)
    assert m.sediment(wp) == PM.ESTATE                                     # never filled
    assert m.upload(inp) is None
    keep = {k: np.array(v) for k, v in m.a.items()}
    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, 6), (5, 1), (3, 3)):
        assert m.sediment(wp, sl0=sl0, n=n) == PM.EINVAL, (sl0, n)
    assert m.sediment(wp, first=1, ntr=2) == PM.EINVAL and m.sediment(wp, first=-1, ntr=1) == PM.EINVAL
    assert m.sediment(wp, first=0, ntr=0) == PM.EINVAL
    assert m.sediment(None) == PM.EINVAL
    assert m.sediment(wp, eb=4) == PM.ESTATE                               # a host form of the other precision
    assert m.sediment(None, eb=4) == PM.EINVAL                             # the NULL comes first
    m.multi = True
    assert m.sediment(wp) == PM.EUNSUPPORTED and m.sediment(wp, sl0=0, n=0) == PM.EINVAL
    assert m.sediment(None) == PM.EUNSUPPORTED                             # the handle comes before the NULL
    m.multi = False
    for k, v in keep.items():
        assert np.array_equal(SM.bits(m.a[k]), SM.bits(v)), k
    s, p = m.sediment(wp)
    assert s.shape == (5, 8, 2) and p.shape == (5, 5, 2) and not np.array_equal(m.a["f"], keep["f"])
    assert np.array_equal(SM.bits(m.a["f"][:, :3]), SM.bits(keep["f"][:, :3]))            # halo columns keep every bit
    assert np.array_equal(SM.bits(m.a["f"][:, 11:]), SM.bits(keep["f"][:, 11:]))
    for k in ("u", "w", "rho", "rhow", "adz", "flux"):
        assert np.array_equal(SM.bits(m.a[k]), SM.bits(keep[k])), k


@pytest.mark.parametrize("boundary", [PM.GIVEN, PM.PERIODIC])
def test_plan_model_sediment_is_export_change_import(oracle, boundary):
    """the call on a block and a tracer = export of the block, the operator, import; on a PERIODIC model the halos of the
    next read-back are wrapped copies of the NEW interior"""
    a, inp = _model(oracle)
    b, _ = _model(oracle)
    for m in (a, b):
        assert m.upload(inp) is None and m.set_boundary(boundary) is None and m.run() is None     # (halos stale)
    wp = SM.make_wp(3, 8, 6, None, np.float64, 7)
    s, p = a.sediment(wp, sl0=1, n=3, first=1, ntr=1)
    exp = b.export_block(1, 3, ("f",), 1, 1)["f"]
    new, s2, p2 = SM.sediment(exp[..., 0], inp["rho"][1:4], inp["adz"][1:4], wp)
    assert b.import_block(1, 3, {"f": new}, 1, 1) is None
    assert np.array_equal(SM.bits(s[..., 0]), SM.bits(s2)) and np.array_equal(SM.bits(p[..., 0]), SM.bits(p2))
    ea, eb = a.export_device(), b.export_device()
    for k in ea:
        assert np.array_equal(SM.bits(ea[k]), SM.bits(eb[k])), k
    if boundary == PM.PERIODIC:
        e = ea["f"]
        assert np.array_equal(SM.bits(e), SM.bits(PM.wrap(np.array(e, order="F"))))
        assert np.array_equal(SM.bits(e[1:4, 3:11, :, 1]), SM.bits(new[:, 3:11]))          # ... of the new interior
    for m in (a, b):
        assert m.run() is None
    ea, eb = a.export_device(), b.export_device()
    for k in ea:
        assert np.array_equal(SM.bits(ea[k]), SM.bits(eb[k])), k


# ---- the interface (files parsed: no device)
def test_python_names(mpdata):
    assert callable(mpdata.sediment) and callable(mpdata.Plan.sediment) and callable(mpdata.Plan.sediment_host)
    assert "sediment" in mpdata.__all__ and "sediment_shapes" in mpdata.__all__
    assert mpdata.sediment_shapes(5, 3, 8) == {"wp": (7, 3, 5), "psfc": (3, 5), "pflux": (7, 5)}
    assert mpdata.sediment_shapes(5, 3, 8, 2) == {"wp": (2, 7, 3, 5), "psfc": (2, 3, 5), "pflux": (2, 7, 5)}


def _c_params(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"header: {name}"
    return [p.strip() for p in m.group(1).split(",")]


def test_header_section():
    hdr = open(os.path.join(ROOT, "include", "mpdata_hip.h")).read()
    sec = hdr.split("---- 3n.")[1].split("---- 4.")[0]
    for word in ("wp", "psfc", "pflux"):
        assert re.search(r"\b" + word + r"\b", sec), word
    assert "windowed plans" in sec.lower() and "are supported" in sec


def test_library_exports_and_ctypes_agree_with_the_header(mpdata):
    hdr = open(os.path.join(ROOT, "include", "mpdata_hip.h")).read()
    L = mpdata.lib()
    ckind = {ctypes.c_int64: "int64_t", ctypes.c_int: "int", ctypes.c_void_p: "*"}
    for n in NAMES:
        params = _c_params(hdr, n)
        fn = getattr(L, n)                                   # the library exports it
        assert fn.restype is ctypes.c_int and fn.argtypes is not None and len(fn.argtypes) == len(params), n
        for a, p in zip(fn.argtypes, params):
            k = ckind[a]
            assert ("*" in p) if k == "*" else (p.startswith(k + " ") and "*" not in p), (n, p, a)


def test_fortran_interface_agrees_with_the_header():
    """the one interface, bound by the literal name, public, the dummy arguments in the header's order, each of the
    header's kind and passed by value"""
    hdr = open(os.path.join(ROOT, "include", "mpdata_hip.h")).read()
    f90 = open(os.path.join(ROOT, "codesign-kernels_amd", "fortran", "mpdata_hip_mod.F90")).read()
    m = re.search(r"integer\(c_int\) function mpdata_plan_sediment_device_c\(([^)]*)\)\s*&?\s*bind\(C, name=\"mpdata_plan_sediment_device\"\)"
                  r"(.*?)end function", f90, re.S)
    assert m
    fargs = [a.strip() for a in m.group(1).replace("&", " ").split(",")]
    params = _c_params(hdr, "mpdata_plan_sediment_device")
    cargs = [re.split(r"[\s*]+", p)[-1] for p in params]
    assert fargs == cargs, (fargs, cargs)
    decl = {}
    for line in m.group(2).splitlines():
        d = re.match(r"\s*(type\(c_ptr\)|integer\(c_int64_t\)|integer\(c_int\))\s*,\s*value\s*::\s*(.*)", line)
        if d:
            for a in d.group(2).split(","):
                decl[a.strip()] = d.group(1)
    for p, a in zip(params, cargs):
        want = "type(c_ptr)" if "*" in p else ("integer(c_int64_t)" if p.startswith("int64_t ") else "integer(c_int)")
        assert decl.get(a) == want, (a, p, decl.get(a))
    assert re.search(r"public ::.*\bmpdata_plan_sediment_device_c\b", f90)
    assert "MPDATA_C_PLAN_SEDIMENT" not in f90 and "MPDATA_C_SEDIMENT" not in f90        # no per-precision macro
    # (its make rule and its .gitignore entry: tests/test_fortran_plan_calls.py, for every program at once)
    assert os.path.exists(os.path.join(ROOT, "tests", "fortran", "sediment_calls.F90"))


def test_argument_errors_without_device(mpdata):
    L = mpdata.lib()
    one = ctypes.c_void_p(8)   # never dereferenced: the checks come before anything looks at the arrays
    for fn in (L.mpdata_sediment_device, L.mpdata_sediment_f32_device):
        assert fn(4, 0, 6, 1, 0, 4, one, one, one, one, None, None, None) == mpdata.EINVAL           # nx < 1
        assert fn(4, 5, 1, 1, 0, 4, one, one, one, one, None, None, None) == mpdata.EINVAL           # nz < 2
        assert b"nz=1" in L.mpdata_last_error()
        assert fn(0, 5, 6, 1, 0, 4, one, one, one, one, None, None, None) == mpdata.EINVAL
        assert fn(4, 5, 6, 0, 0, 4, one, one, one, one, None, None, None) == mpdata.EINVAL
        for sl0, n in ((0, 0), (-1, 2), (0, 5), (4, 1), (2, 3)):
            assert fn(4, 5, 6, 1, sl0, n, one, one, one, one, None, None, None) == mpdata.EINVAL, (sl0, n)
            assert b"outside" in L.mpdata_last_error()
        for i, nm in enumerate(("f", "rho", "adz", "wp")):
            args = [one, one, one, one]
            args[i] = None
            assert fn(4, 5, 6, 1, 0, 4, *args, None, None, None) == mpdata.EINVAL, nm
            assert b"null " + nm.encode() in L.mpdata_last_error()
        assert fn(4, 5, 1, 1, 0, 4, None, None, None, None, None, None, None) == mpdata.EINVAL and b"nz=1" in L.mpdata_last_error()
        assert fn(4, 5, 6, 1, 0, 4, one, None, one, None, None, None, None) == mpdata.EINVAL and b"null rho" in L.mpdata_last_error()
    assert L.mpdata_plan_sediment_device(None, 0, 1, one, None, None, 0, 1) == mpdata.EINVAL
    assert b"null plan" in L.mpdata_last_error()
    assert L.mpdata_plan_sediment(None, 0, 1, one, None, None) == mpdata.EINVAL
    assert L.mpdata_plan_sediment_f32(None, 0, 1, one, None, None) == mpdata.EINVAL
    for n, sl0 in ((0, 0), (-2, 0), (1, -1)):   # (checked before the plan is looked at)
        assert L.mpdata_plan_sediment_device(one, sl0, n, one, None, None, 0, 1) == mpdata.EINVAL
    assert L.mpdata_plan_sediment_device(one, 0, 0, None, None, None, 0, 1) == mpdata.EINVAL
    assert b"null wp" not in L.mpdata_last_error()                                  # the range came first


def test_new_kernels_do_not_spill_and_fit_the_lds_budget():
    """the resource-usage report the build writes next to the object of mpdata_sediment.hip: no scratch memory, no vector
    and no scalar register spilled in any kernel; the LDS of the plan-layout kernel is dynamic, its budget a constant of
    the file: 40 KiB at most, four workgroups per CU"""
    csrc = os.path.join(ROOT, "codesign-kernels_amd", "csrc")
    rep = os.path.join(csrc, "mpdata_sediment.usage.txt")
    if not os.path.exists(rep):
        pytest.skip("no resource-usage report (library not built here)")
    txt = open(rep).read()
    assert len(re.findall(r"Function Name: \S*wm_sediment_kernel", txt)) == 5      # f64 and f32, plain and windowed; f32 in reals
    assert len(re.findall(r"Function Name: \S*wm_sediment_psfc_kernel", txt)) == 2
    assert len(re.findall(r"Function Name: \S*ref_sediment_kernel", txt)) == 2
    assert len(re.findall(r"Function Name: \S*ref_sediment_store_kernel", txt)) == 2
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", txt)]
    assert len(scratch) == 11 and set(scratch) == {0}
    assert {int(x) for x in re.findall(r"VGPRs Spill: (\d+)", txt)} == {0}
    assert {int(x) for x in re.findall(r"SGPRs Spill: (\d+)", txt)} == {0}
    src = open(os.path.join(csrc, "mpdata_sediment.hip")).read()
    walk = open(os.path.join(csrc, "mpdata_wm_walk.h")).read()
    m = re.search(r"constexpr int LDS_ELEMS = (\d+);", walk)                               # (the one statement of the limit)
    assert m and int(m.group(1)) * 8 <= 40 * 1024
    assert "col_groups_tiled(j, b.sel, wg, LDS_ELEMS," in src and "g->lds_e <= budget" in walk     # the launch refuses more
